"""CPU: the scalar model's sequence trace (wave_model.trace, lz4w_trace in tests/sim/wave_encoder_model.c) is the parse that
wave_model.compress serialises, and the shape corpus (tests/wave_shapes.py) makes the model write every sequence shape that the
throughput encoder's kernel writes in a place of its own, under every configuration that moves segment and window starts."""
import pytest

import oracle_api as O
import test_wave_model
import wave_model as W
import wave_shapes as S

TRACE_CONFIGS = [dict(sub=1), dict(sub=2), dict(sub=3), dict(sub=4), dict(slide=0), dict(slide=1), dict(slide=2)]


def _check_trace(data, kw):
    seqs, segs = W.trace(data, **kw)
    assert W.serialise(data, seqs) == W.compress(data, **kw), kw
    if not data:
        assert len(seqs) == 0
        return
    hist = kw.get("hist", 0)
    # the sequences tile the block behind the history, and every segment-first / lane / call field is where the kernel puts it
    pos = hist
    for k, s in enumerate(seqs):
        assert s["lit_start"] == pos, (k, kw)
        pos += int(s["lit_len"]) + int(s["mlen"])
        assert (s["mlen"] == 0) == (k == len(seqs) - 1)
        if s["mlen"] and not s["run"]:
            assert s["mlen"] >= 4 and 1 <= s["off"] <= 65535 and s["lane"] < 64
            if k and seqs[k - 1]["mlen"] and (seqs[k - 1]["win"], seqs[k - 1]["wj"]) == (s["win"], s["wj"]):
                prev = seqs[k - 1]
                assert not s["first"]
                assert (s["call"], s["lane"]) in ((prev["call"], prev["lane"] + 1), (prev["call"] + 1, 0)), (k, kw)
            else:
                assert s["first"] and s["call"] == 0 and s["lane"] == 0, (k, kw)
        if s["first"]:
            seg = [g for g in segs if (g["win"], g["wj"]) == (s["win"], s["wj"])]
            assert len(seg) == 1 and s["lit_start"] + s["pend"] == seg[0]["s0"] and s["pend"] <= s["lit_len"], (k, kw)
    assert pos == len(data)
    for g in segs:
        assert g["s0"] < g["s1"] <= len(data) and g["wbase"] <= g["s0"]


@pytest.mark.parametrize("i", range(len(test_wave_model.inputs())))
def test_trace_serialises_to_the_model_bytes(i):
    data = test_wave_model.inputs()[i]
    for kw in TRACE_CONFIGS:
        _check_trace(data, kw)
    if len(data) > W.HIST:
        _check_trace(data, dict(hist=W.HIST))


@pytest.mark.parametrize("config", sorted(S.CONFIGS))
def test_shape_corpus_trace_and_oracle(config):
    """every corpus block: the trace re-serialises to the model's bytes, and lz4_flex's decoder (the oracle) decodes those"""
    for data, kw in S.blocks(config):
        _check_trace(data, kw)
        comp = W.compress(data, **kw)
        hist = kw.get("hist", 0)
        assert O.decompress(comp, len(data) - hist, dict_data=data[:hist] if hist else None) == ("ok", data[hist:])


@pytest.mark.parametrize("config", sorted(S.CONFIGS))
def test_shape_corpus_coverage(config):
    """the model's output of the corpus holds every class of wave_shapes.REQUIRED (a change to the parse that loses one fails here,
    naming it)"""
    got = S.coverage(config)
    missing = [c for c in S.required(config) if c not in got]
    assert not missing, "config %s: the shape corpus no longer produces: %s" % (config, "; ".join(missing))
