"""compress_mode 2 ("high") with "compress_high_linked" 1: a block with h bytes of its own stream in front of it (LZ4FLEX_BLOCK_HISTORY, a
Linked frame's blocks) is a block whose dictionary is those bytes -- tests/sim/high_dict_model.c composed over a stream.  Python glue
only; test infrastructure."""
import hc_dict_model as D

HISTORY = 32768          # what the definition reads of the bytes in front of a block
DEPTH_DEFAULT = D.DEPTH_DEFAULT

_memo = {}


def block(stream, at, n, h, depth=DEPTH_DEFAULT):
    """the bytes of stream[at : at + n] with the h bytes in front of it as its history"""
    assert 0 <= h <= at
    data = bytes(stream[at:at + n])
    hist = bytes(stream[at - min(h, HISTORY):at]) if h >= 4 else b""
    key = (data, hist, depth)
    if key not in _memo:
        _memo[key] = D.compress(data, hist, depth)
    return _memo[key]


def blocks(stream, cut, depth=DEPTH_DEFAULT, linked=True):
    """the stream cut into blocks of `cut` bytes: every block's bytes, each behind everything in front of it (linked) or alone"""
    return [block(stream, at, min(cut, len(stream) - at), at if linked else 0, depth) for at in range(0, len(stream), cut)]


def frame_payloads(stream, cut, depth=DEPTH_DEFAULT, linked=True):
    """what a frame with blocks of `cut` bytes carries per block: (payload, stored raw?) -- frame/compress.rs:301-306"""
    out = []
    for k, m in enumerate(blocks(stream, cut, depth, linked)):
        raw = bytes(stream[k * cut:(k + 1) * cut])
        out.append((m, False) if len(m) < len(raw) else (raw, True))
    return out
