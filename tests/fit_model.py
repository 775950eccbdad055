"""The fit rule of lz4flex_fit_batch (include/lz4flex_amd.h, lz4_fit.hip) as plain Python: a finished LZ4 block cut to a capacity -- liblz4's
LZ4_compress_destSize as a pass over the block.  Test infrastructure (a plain module, not a fixture): the GPU tests compare the kernels
with fit() byte for byte, the CPU tests compare fit() with brute_force(), which enumerates every (k, m', L) instead of computing them.

A block B has sequences j = 0 .. S-1 (literals l_j, match m_j, offset d_j; the last one has no match), c_j is the compressed offset of
sequence j's token and p_j the decoded offset of its first byte; B decodes to the n bytes of `src`.
    ext(x)  = 0 if x < 15 else 1 + (x - 15) // 255          the length bytes behind a token's nibble
    tail(L) = 1 + ext(L) + L                                a final run of L literals, compressed
    Lfit(r, avail) = the largest L in [0, avail] with tail(L) <= r
Every sequence whose token lies in front of `cap` (c_k < cap) is parsed, in the reference's check order (decompress.rs:249-443), and is a
place to cut; the first error met there is the block's status.  What lies behind is not looked at."""

OK, E_OUTPUT_TOO_SMALL, E_LITERAL_OUT_OF_BOUNDS, E_EXPECTED_ANOTHER_BYTE, E_OFFSET_ZERO, E_OFFSET_OUT_OF_BOUNDS = 0, 1, 2, 3, 4, 5
PLAIN, CLIPPED = 1, 0          # the last field of a candidate's key: Plain before Clipped


def ext(x):
    return 0 if x < 15 else 1 + (x - 15) // 255


def tail(L):
    return 1 + ext(L) + L


def lfit(r, avail):
    """the largest L in [0, avail] with tail(L) <= r, in closed form (r >= 1); -1 when avail < 0"""
    if avail < 0:
        return -1
    if r <= 16:
        L = min(r - 1, 14)
    else:
        y = r - 17                       # L = 15 + x with x + x // 255 <= y
        L = 15 + y - y // 256 - (1 if y % 256 == 255 else 0)
    return min(L, avail)


class BlockError(Exception):
    def __init__(self, code):
        super().__init__(code)
        self.code = code


def _length(B, ip, v):
    """read_integer (decompress.rs:160-174)"""
    while True:
        if ip >= len(B):
            raise BlockError(E_EXPECTED_ANOTHER_BYTE)
        e = B[ip]
        ip += 1
        v += e
        if e != 255:
            return ip, v


def sequences(B, cap):
    """the sequences of B whose token lies in front of cap: (c, p, l, m, d) each, m = 0 for the block's last one; BlockError for the first
    error the reference would meet among them"""
    B = bytes(B)
    ip = op = 0
    while ip < cap:
        if ip >= len(B):
            raise BlockError(E_EXPECTED_ANOTHER_BYTE)          # (the empty block, :207-209; else :439-443 has caught it)
        c, p = ip, op
        token = B[ip]
        ip += 1
        lit = token >> 4
        if lit == 15:
            ip, lit = _length(B, ip, lit)
        if lit > len(B) - ip:
            raise BlockError(E_LITERAL_OUT_OF_BOUNDS)
        ip += lit
        op += lit
        if ip >= len(B):
            yield (c, p, lit, 0, 0)
            return
        if len(B) - ip < 2:
            raise BlockError(E_EXPECTED_ANOTHER_BYTE)
        d = B[ip] | (B[ip + 1] << 8)
        ip += 2
        if d == 0:
            raise BlockError(E_OFFSET_ZERO)
        ml = 4 + (token & 15)
        if ml == 19:
            ip, ml = _length(B, ip, ml)
        if d > op:
            raise BlockError(E_OFFSET_OUT_OF_BOUNDS)
        op += ml
        if ip >= len(B):
            raise BlockError(E_EXPECTED_ANOTHER_BYTE)
        yield (c, p, lit, ml, d)


def _lmin(m_prev):
    """the format's end rules for a final run behind a match of m_prev bytes (None: no match in front of it): the last 5 bytes are
    literals, the last match starts at least 12 bytes before the end"""
    return 0 if m_prev is None else max(5, 12 - m_prev)


def candidates(seqs, n, cap):
    """the rule's candidates: (used, cap - size, -k, form, k, m', L), the best one is the maximum"""
    for k, (c, p, l, m, d) in enumerate(seqs):
        L = lfit(cap - c, n - p)
        if L >= _lmin(seqs[k - 1][3] if k else None):
            yield (p + L, cap - (c + tail(L)), -k, PLAIN, k, 0, L)
        if m >= 5:
            h = 1 + ext(l) + l + 2
            b = cap - c - h - 1
            if b < 5:
                continue
            mc = min(m - 1, 18 + 255 * (b - 5))
            if max(5, 12 - mc) > b:
                continue
            L = lfit(cap - c - h - ext(mc - 4), n - p - l - mc)
            if L >= max(5, 12 - mc):
                yield (p + l + mc + L, cap - (c + h + ext(mc - 4) + tail(L)), -k, CLIPPED, k, mc, L)


def brute_candidates(seqs, n, cap):
    """the same set by enumeration: every k, every clipped match length m' and every final run L that the capacity, the source and the
    end rules allow -- per (k, form, m') the longest L; Clipped(k) at the rule's m' only is what candidates() must equal, every other m'
    is there to show that none of them is better"""
    for k, (c, p, l, m, d) in enumerate(seqs):
        lmin = _lmin(seqs[k - 1][3] if k else None)
        best = None
        for L in range(0, max(n - p, -1) + 1):
            if c + tail(L) > cap:
                break
            if L >= lmin:
                best = L
        if best is not None:
            yield (p + best, cap - (c + tail(best)), -k, PLAIN, k, 0, best)
        if m >= 5:
            h = 1 + ext(l) + l + 2
            for mc in range(4, m):
                lmin = max(5, 12 - mc)
                best = None
                for L in range(0, max(n - p - l - mc, -1) + 1):
                    if c + h + ext(mc - 4) + tail(L) > cap:
                        break
                    if L >= lmin:
                        best = L
                if best is not None:
                    yield (p + l + mc + best, cap - (c + h + ext(mc - 4) + tail(best)), -k, CLIPPED, k, mc, best)


def _len_bytes(v):
    out = bytearray()
    while v >= 255:
        out.append(255)
        v -= 255
    out.append(v)
    return bytes(out)


def _final_run(lits):
    L = len(lits)
    return bytes([min(L, 15) << 4]) + (_len_bytes(L - 15) if L >= 15 else b"") + bytes(lits)


def emit(B, src, seqs, cand):
    """the block of a candidate"""
    used, _slack, _nk, form, k, mc, L = cand
    c, p, l, m, d = seqs[k]
    out = bytearray(B[:c])
    if form == CLIPPED:
        h = 1 + ext(l) + l + 2
        out.append((B[c] & 0xF0) | min(mc - 4, 15))
        out += B[c + 1:c + h]
        if mc - 4 >= 15:
            out += _len_bytes(mc - 19)
    out += _final_run(src[used - L:used])
    return bytes(out)


def fit(B, src, cap, chooser=candidates):
    """(out, in_used, status) of block B, which decodes to src, cut to cap bytes"""
    B, src = bytes(B), bytes(src)
    if len(B) <= cap:
        return B, len(src), OK
    try:
        seqs = list(sequences(B, cap))
    except BlockError as e:
        return b"", 0, e.code
    cands = list(chooser(seqs, len(src), cap))
    if not cands:
        return b"", 0, E_OUTPUT_TOO_SMALL
    best = max(cands, key=lambda t: t[:4] + (t[5],))     # (the brute force's ties: the longest clipped match, the rule's)
    out = emit(B, src, seqs, best)
    assert len(out) == cap - best[1] <= cap
    return out, best[0], OK


def brute_force(B, src, cap):
    """fit() with the candidates enumerated; its winner may clip a match to another m' than the rule's only if that were strictly better"""
    return fit(B, src, cap, chooser=brute_candidates)
