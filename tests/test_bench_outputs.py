"""CPU: bench.py --dump-outputs' arrays (digests, seeded samples, the size bound) on host tensors"""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench as B  # noqa: E402


def _blocks(n=300, stride=72128, seed=0):
    g = torch.Generator().manual_seed(seed)
    comp = torch.randint(0, 256, (n * stride,), dtype=torch.uint8, generator=g)
    clen = torch.randint(1, stride + 1, (n,), dtype=torch.int32, generator=g)
    back = torch.randint(0, 256, (n * B.BLOCK,), dtype=torch.uint8, generator=g)
    blen = torch.full((n,), B.BLOCK, dtype=torch.int32)
    st = torch.zeros(n, dtype=torch.int32)
    return n, stride, comp, clen, st, back, blen, st


def test_block_outputs_digests_and_samples():
    n, stride, comp, clen, cst, back, blen, dst = _blocks()
    o = B.block_outputs("both", n, stride, comp, clen, cst, back, blen, dst)
    assert all(a.dtype in (np.float32, np.float64) for a in o.values())
    for r in (0, 7, n - 1):
        x = comp[r * stride:r * stride + int(clen[r])].numpy().astype(np.int64)
        assert o["compressed_digest"][r] == float((x * np.arange(1, len(x) + 1)).sum())
        y = back[r * B.BLOCK:(r + 1) * B.BLOCK].numpy().astype(np.int64)
        assert o["decompressed_digest"][r] == float((y * np.arange(1, B.BLOCK + 1)).sum())
    idx = o["sample_blocks"].astype(np.int64)
    assert len(idx) == B.DUMP_SAMPLE and (np.diff(idx) > 0).all()
    want = np.concatenate([comp[i * stride:i * stride + int(clen[i])].numpy() for i in idx])
    assert np.array_equal(o["compressed_sample"], want.astype(np.float32))
    assert np.array_equal(o["decompressed_sample"][3], back[idx[3] * B.BLOCK:(idx[3] + 1) * B.BLOCK].numpy().astype(np.float32))
    o2 = B.block_outputs("both", *_blocks())
    assert all(np.array_equal(o[k], o2[k]) for k in o)                   # same inputs, same sample


def test_byte_outputs_pads_past_the_end():
    data = bytes(range(256)) * 1000                                      # 256 000 bytes: 4 chunks, the last one partial
    o = B.byte_outputs("frame", data)
    assert o["frame_len"].tolist() == [len(data)] and o["frame_digest"].shape == (4,)
    tail = len(data) - 3 * B.BLOCK
    assert np.array_equal(o["frame_sample"][3, :tail], np.frombuffer(data[3 * B.BLOCK:], dtype=np.uint8).astype(np.float32))
    assert (o["frame_sample"][3, tail:] == -1).all()


def test_write_outputs_bound(tmp_path):
    B.write_outputs(str(tmp_path / "ok"), {"a": np.zeros(10, dtype=np.float32)})
    assert np.array_equal(np.load(tmp_path / "ok" / "a.npy"), np.zeros(10, dtype=np.float32))
    with pytest.raises(AssertionError):
        B.write_outputs(str(tmp_path / "big"), {"a": np.zeros(B.DUMP_LIMIT // 8 + 1, dtype=np.float64)})
    assert not (tmp_path / "big").exists()
