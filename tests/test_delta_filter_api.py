"""CPU test of LZ4FLEX_FILTER_DELTA on the typed batch entries (lz4flex_filter_batch, lz4flex_compress_batch_typed,
lz4flex_decompress_batch_typed): the define, its Python twin and the definition in the header; the ABI number stays; the flag is a valid
`filter` with each of the three base filters and nothing else is; the checks answer before a context or a device is looked at; the
Python keyword `delta` is a bool.  No compute calls."""
import re

import numpy as np
import pytest

from test_filter_api import CALLS, HEADER, _args, _compress, _decompress, _filter, lib      # noqa: F401  (lib: the fixture)

FLAGGED = (0x10, 0x11, 0x12)


def test_the_define_and_the_definition(lib):
    from lz4_flex_amd import _lib, block
    text = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"#define\s+LZ4FLEX_FILTER_DELTA\s+0x10\b", src) and re.search(r"#define\s+LZ4FLEX_DELTA_RESTART\s+1024\b", src)
    assert _lib.FILTER_DELTA == 0x10
    assert block.FILTERS == {"none": 0, "shuffle": 1, "bitshuffle": 2}
    assert lib.lz4flex_abi_version() == 8
    note = text[text.index("The round of this header: 8"):text.index("int lz4flex_abi_version(void);")]
    assert "LZ4FLEX_FILTER_DELTA" in note and "LZ4FLEX_DELTA_RESTART" in note
    typed = text[text.index("---- typed batches"):text.index("#define LZ4FLEX_FILTER_NONE")]
    for line in ("`d[e] = x[e]` where `e % LZ4FLEX_DELTA_RESTART == 0`", "`d[e] = (x[e] - x[e-1]) mod 2^(8E)`",
                 "`x[e] = (d[r] + ... + d[e]) mod 2^(8E)` with `r = e - e % LZ4FLEX_DELTA_RESTART`", "0, 1, 2, 0x10, 0x11 and 0x12",
                 "`01 00 03 00 02 00 AA` becomes `01 00 02 00 FF FF AA`", "5, then 1 023 zeros, then 5, then 0"):
        assert line in typed, line


def test_the_flag_is_a_valid_filter_and_nothing_else_is(lib):
    from lz4_flex_amd import _lib
    INV, NODEV = -_lib.E_INVALID_ARG, -_lib.E_NO_DEVICE
    HOST, DEV, BIG = _lib.MEM_HOST, _lib.MEM_DEVICE, _lib.MEM_BIG_BLOCKS
    a = _args()
    for what, call, arrays in CALLS:
        for mem in (HOST, DEV, HOST | BIG, DEV | BIG):
            for filt in FLAGGED:
                for elem in (1, 2, 4, 8):
                    assert call(lib, a, n=0, filt=filt, elem=elem, mem=mem) == 0, (what, hex(filt), elem, mem)
                assert call(lib, a, n=0, filt=filt, elem=3, mem=mem) == INV and call(lib, a, filt=filt, elem=16, mem=mem) == INV
                for name in arrays:
                    assert call(lib, a, filt=filt, mem=mem, **{name: None}) == INV, (what, hex(filt), name)
            for filt in (0x13, 0x14, 0x20, 0x30, 0x110, -0x10, 0x10 - (1 << 31)):
                assert call(lib, a, filt=filt, mem=mem) == INV and call(lib, a, n=0, filt=filt, mem=mem) == INV, (what, hex(filt))
    # the tmp slots: the flag alone is a filter, so a DEVICE compress or decompress needs them; a HOST call does not look at them
    for call in (_compress, _decompress):
        for filt in FLAGGED:
            assert call(lib, a, filt=filt, mem=DEV, tmp=None) == INV and call(lib, a, filt=filt, mem=DEV | BIG, tmp_off=None) == INV, hex(filt)
    assert (a["out_len"][0], a["status"][0], a["detail"][0], a["out"].raw) == (7, 7, 7, b"\xC5" * 64)
    if lib.lz4flex_device_count() == 0:
        for what, call, _arrays in CALLS:
            for filt in FLAGGED:
                for elem in (1, 2, 4, 8):
                    assert call(lib, a, filt=filt, elem=elem) == NODEV, (what, hex(filt), elem)
                assert call(lib, a, filt=filt, mem=HOST, tmp=None, tmp_off=None) == NODEV, what
        assert _filter(lib, a, filt=0x10, inverse=1) == NODEV
        assert (a["out_len"][0], a["status"][0], a["out"].raw) == (7, 7, b"\xC5" * 64)


def test_the_python_keyword_is_a_bool(lib):
    import inspect

    import torch
    from lz4_flex_amd import block
    for name in ("filter_batch", "compress_batch_typed", "decompress_batch_typed", "filter_blocks_device", "compress_blocks_typed_device",
                 "decompress_blocks_typed_device", "compress_tensor"):
        assert inspect.signature(getattr(block, name)).parameters["delta"].default is False, name
    x, out = np.arange(16, dtype=np.uint8), np.zeros(64, np.uint8)
    for delta in (1, 0, None, "yes", 0x10, np.True_):
        with pytest.raises(ValueError):
            block.filter_batch(x, [0], [16], out, [0], "shuffle", 2, delta=delta)
        with pytest.raises(ValueError):
            block.compress_batch_typed(x, [0], [16], out, [0], [64], "none", 2, delta=delta)
        with pytest.raises(ValueError):
            block.decompress_batch_typed(x, [0], [16], out, [0], [64], 2, 8, delta=delta)
    assert block._filter_args("bitshuffle", 8, True) == (0x12, 8) and block._filter_args(0, 1, True) == (0x10, 1)
    assert block._filter_args("shuffle", 4, False) == (1, 4) and block._filter_args("shuffle", 4) == (1, 4)
    # the flag is not a filter name or id of its own
    for filt in ("delta", 0x10, 0x11, 0x12):
        with pytest.raises(ValueError):
            block.filter_batch(x, [0], [16], out, [0], filt, 2, delta=True)
    if lib.lz4flex_device_count() == 0:                  # accepted: the call gets as far as the missing device
        for delta in (True, False):
            with pytest.raises(block.DeviceError):
                block.filter_batch(x, [0], [16], out, [0], "none", 2, delta=delta)
            with pytest.raises(block.DeviceError):
                block.compress_batch_typed(x, [0], [16], out, [0], [64], "bitshuffle", 4, delta=delta)
            with pytest.raises(block.DeviceError):
                block.decompress_batch_typed(x, [0], [16], out, [0], [64], 2, 8, delta=delta)
    rec = block.CompressedTensor(None, None, None, (3,), torch.int64, 4096, 2)
    assert rec.delta is False and rec.filter == 2
    assert block.CompressedTensor(None, None, None, (3,), torch.int64, 4096, 2, True).delta is True
    host = torch.zeros(64, dtype=torch.int64)
    with pytest.raises(ValueError):
        block.compress_tensor(host, delta=True)          # (not on the GPU)
