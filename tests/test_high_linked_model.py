"""CPU: compress_mode 2 ("high") over a stream's history ("compress_high_linked" 1) -- the composed definition
(tests/hc_linked_model.py over tests/sim/high_dict_model.c): the known answers at depth 16, the history's edges, and the oracle decodes
every block with the stream in front of it as its dictionary."""
import pytest

import hc_linked_model as K
import hc_model as H
import oracle_api as O


def J():
    return O.fixture_plain("compression_66k_JSON")


def T():
    return O.fixture_plain("compression_65k")


def streams():
    j, t, k = J(), T(), O.fixture_plain("compression_34k")
    return {"j4": (j * 4)[:3 * 65536 + 17], "jtk": j + t + k, "t": t, "j": j}


KNOWN = [
    ("j4", 65536, [12629, 12739, 12704, 19], [12629, 11962, 11966, 11]),
    ("jtk", 65536, [12629, 30299, 16585], [12629, 29879, 14972]),
    ("t", 16384, [8964, 8463, 9026, 8821], [8964, 6865, 6987, 7376]),
    ("j", 16384, [4755, 3552, 2996, 3115, 572], [4755, 3182, 2364, 2380, 220]),
]


@pytest.mark.parametrize("k", range(len(KNOWN)))
def test_known_answers(k):
    name, cut, independent, linked = KNOWN[k]
    s = streams()[name]
    ind = K.blocks(s, cut, 16, linked=False)
    assert ind == [H.compress(s[at:at + cut], 16) for at in range(0, len(s), cut)]
    assert [len(b) for b in ind] == independent
    got = K.blocks(s, cut, 16)
    assert [len(b) for b in got] == linked
    for i, b in enumerate(got):
        at = i * cut
        raw = s[at:at + cut]
        assert O.decompress(b, len(raw), dict_data=s[max(0, at - 65536):at] or None) == ("ok", raw), i


def test_the_last_17_bytes_are_compressed_in_a_linked_frame():
    s = streams()["j4"]
    assert K.frame_payloads(s, 65536, 16, linked=False)[3] == (s[-17:], True)
    assert K.frame_payloads(s, 65536, 16)[3] == (K.block(s, 3 * 65536, 17, 3 * 65536, 16), False)


EDGES = ((0, 1273), (1, 1273), (3, 1273), (4, 1269), (5, 1268), (11, 1265), (12, 1264), (4095, 767), (32767, 726), (32768, 726),
         (32769, 726), (40000, 726))


def test_history_edges():
    j = J()
    assert [len(K.block(j, 40000, 5000, h, 16)) for h, _ in EDGES] == [n for _, n in EDGES]
    plain = H.compress(j[40000:45000], 16)
    for h in (0, 1, 3):
        assert K.block(j, 40000, 5000, h, 16) == plain
    # more than 32 KiB in front: the bytes are those of the last 32 KiB
    assert K.block(j, 40000, 5000, 32769, 16) == K.block(j, 40000, 5000, 40000, 16) == K.block(j, 40000, 5000, 32768, 16)


def test_the_log_stream_totals():
    from lz4_flex_amd import workloads
    log = bytes(workloads.log_stream(0, 1 << 20).numpy())
    assert sum(len(b) for b in K.blocks(log, 65536, 16, linked=False)) == 274737
    assert sum(len(b) for b in K.blocks(log, 65536, 16)) == 259660
