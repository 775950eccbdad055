"""The numpy model of the typed batches' filters (include/lz4flex_amd.h, "typed batches"), written from the definition.  A block is L
bytes, E the element size (1, 2, 4, 8); both filters map L bytes to L bytes.
  SHUFFLE:     m = L // E; out[j * m + e] = in[e * E + j]; the last L - m * E bytes stay where they are.
  BITSHUFFLE:  m8 = L // E // 8 * 8; plane p = 8 j + k holds bit k (LSB = 0) of byte j of every element and occupies out[p * m8 / 8 ..
               (p + 1) * m8 / 8); bit b of byte q of plane p is bit k of in[(8 q + b) * E + j]; the last L - m8 * E bytes stay.
A plain module, not a fixture."""
import numpy as np

NONE, SHUFFLE, BITSHUFFLE = 0, 1, 2
ELEMS = (1, 2, 4, 8)


def _u8(x):
    return np.frombuffer(bytes(x), np.uint8) if not isinstance(x, np.ndarray) else np.ascontiguousarray(x, np.uint8).reshape(-1)


def shuffle(x, E):
    x = _u8(x)
    m = x.size // E
    out = x.copy()
    out[:m * E] = x[:m * E].reshape(m, E).T.reshape(-1)
    return out


def unshuffle(y, E):
    y = _u8(y)
    m = y.size // E
    out = y.copy()
    out[:m * E] = y[:m * E].reshape(E, m).T.reshape(-1)
    return out


def bitshuffle(x, E):
    x = _u8(x)
    m8 = x.size // E // 8 * 8
    out = x.copy()
    if m8:
        bits = np.unpackbits(x[:m8 * E].reshape(m8, E), axis=1, bitorder="little")          # [element, 8 j + k]
        out[:m8 * E] = np.packbits(bits.T, axis=1, bitorder="little").reshape(-1)           # [plane, q]
    return out


def unbitshuffle(y, E):
    y = _u8(y)
    m8 = y.size // E // 8 * 8
    out = y.copy()
    if m8:
        bits = np.unpackbits(y[:m8 * E].reshape(8 * E, m8 // 8), axis=1, bitorder="little")  # [plane, element]
        out[:m8 * E] = np.packbits(bits.T, axis=1, bitorder="little").reshape(-1)            # [element, byte]
    return out


def forward(x, filt, E):
    return {NONE: lambda a, _e: _u8(a).copy(), SHUFFLE: shuffle, BITSHUFFLE: bitshuffle}[filt](x, E)


def inverse(y, filt, E):
    return {NONE: lambda a, _e: _u8(a).copy(), SHUFFLE: unshuffle, BITSHUFFLE: unbitshuffle}[filt](y, E)


def apply(x, filt, E, inv=False):
    return inverse(x, filt, E) if inv else forward(x, filt, E)


# ---- the workloads the feature is for (seeded, generated where they are used) ---------------------------------------------------------
def bf16_weights(n_bytes, seed):
    """bf16 N(0, 0.02): fp32 rounded to nearest even, as bytes"""
    w = (np.random.default_rng(seed).standard_normal(n_bytes // 2) * 0.02).astype(np.float32).view(np.uint32)
    r = (w + np.uint32(0x7FFF) + ((w >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)
    return r.astype(np.uint16).view(np.uint8)


def int64_timestamps(n_bytes, seed):
    """the cumulative sum of integers in [900, 1100) plus 1.7e12, as bytes"""
    steps = np.random.default_rng(seed).integers(900, 1100, n_bytes // 8).astype(np.int64)
    return (np.cumsum(steps) + np.int64(1_700_000_000_000)).view(np.uint8)
