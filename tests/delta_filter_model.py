"""The numpy model of the delta stage of typed batches (include/lz4flex_amd.h, "typed batches": LZ4FLEX_FILTER_DELTA), written from the
definition and composed with filter_model.  A block is L bytes, E the element size, m = L // E; x[e] is the little-endian unsigned integer
at in[e * E]:
  forward:  d[e] = x[e] where e % 1024 == 0, else (x[e] - x[e - 1]) mod 2^(8 E); the last L - m * E bytes stay; then the base filter over d.
  inverse:  the base filter's inverse, then x[e] = (d[r] + ... + d[e]) mod 2^(8 E), r = e - e % 1024.
A plain module, not a fixture."""
import numpy as np

import filter_model as M

DELTA = 0x10
RESTART = 1024
UINT = {1: np.uint8, 2: np.dtype("<u2"), 4: np.dtype("<u4"), 8: np.dtype("<u8")}


def delta(x, E):
    x = M._u8(x)
    m = x.size // E
    out = x.copy()
    if m:
        v = x[:m * E].view(UINT[E])
        d = v.copy()
        d[1:] = v[1:] - v[:-1]                           # (unsigned numpy arithmetic wraps mod 2^(8 E))
        d[::RESTART] = v[::RESTART]
        out[:m * E] = d.view(np.uint8)
    return out


def undelta(y, E):
    y = M._u8(y)
    m = y.size // E
    out = y.copy()
    if m:
        d = y[:m * E].view(UINT[E])
        v = np.empty_like(d)
        for r in range(0, m, RESTART):
            v[r:r + RESTART] = np.cumsum(d[r:r + RESTART], dtype=d.dtype)
        out[:m * E] = v.view(np.uint8)
    return out


def forward(x, base, E, delta_on=True):
    return M.forward(delta(x, E) if delta_on else x, base, E)


def inverse(y, base, E, delta_on=True):
    x = M.inverse(y, base, E)
    return undelta(x, E) if delta_on else x
