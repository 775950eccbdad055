"""CPU: the generated gfx950 ISA of the shared-dictionary encoder path.  tests/test_isa_checks.py looks at the FIRST function whose
name starts with index_window; index_window and run_scan are templates now, and the instance that carries the digest's table loads in
front of the counted-wait pipeline (index_window<true>) must be as clean as the other one."""
import re

import pytest


@pytest.fixture(scope="module")
def isa():
    from lz4_flex_amd import build
    return build.wave_isa()


def _functions(isa, stem):
    text = "\n".join(isa)
    return {m.group(1): m.group(0).splitlines()
            for m in re.finditer(r"^(_ZN11lz4flex_dev4wave\d+%s\w*):.*?^\.Lfunc_end\d+:" % stem, text, re.S | re.M)}


def test_every_index_window_instance_is_free_of_spill_stores_inside_its_loops(isa):
    fns = _functions(isa, "index_window")
    assert len(fns) == 2 and any("ILb1E" in n for n in fns) and any("ILb0E" in n for n in fns), sorted(fns)
    for name, body in fns.items():
        loops = [i for i, l in enumerate(body) if "Loop Header" in l]
        assert loops, name
        first_loop, last_branch = loops[0], max(i for i, l in enumerate(body) if "s_cbranch" in l)
        stores = [l.strip() for i, l in enumerate(body) if first_loop < i < last_branch and "scratch_store" in l]
        assert not stores, (name, stores[:5])


def test_run_scan_instances_use_no_scratch(isa):
    fns = _functions(isa, "run_scan")
    assert len(fns) == 2, sorted(fns)
    for name, body in fns.items():
        assert not any("scratch_" in l for l in body), name


def test_shared_instance_holds_the_pipeline_and_the_table_loads(isa):
    """index_window<true> has the same marked loads and counted waits as index_window<false>, and its eight 16-byte table loads"""
    from lz4_flex_amd import build
    fns = _functions(isa, "index_window")
    t = next(b for n, b in fns.items() if "ILb1E" in n)
    f = next(b for n, b in fns.items() if "ILb0E" in n)
    count = lambda body, mark: sum(1 for l in body if mark in l)      # noqa: E731
    assert count(t, "lz4w-load") == count(f, "lz4w-load") >= 16
    # (the first-KiB run test of the ordinary path has one counted wait and four drains of its own; the shared path asks the digest)
    assert count(f, "lz4w-wait") - 5 <= count(t, "lz4w-wait") <= count(f, "lz4w-wait")
    ok, msg, _l, _w = build.check_async_loads(t)
    assert ok, msg
    plain = [l for l in t if "global_load_dwordx4" in l and "lz4w-load" not in l]
    assert len(plain) >= 8


def test_all_encoder_kernels_keep_two_workgroups_per_cu(isa):
    """80 VGPRs: twelve wavefronts per workgroup, two workgroups per CU"""
    text = "\n".join(isa)
    got = dict(re.findall(r"\.name:\s+_ZN11lz4flex_dev4wave\d+(lz4_compress_wave\w*?kernel)E\w*\n(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)", text))
    assert set(got) == {"lz4_compress_wave_kernel", "lz4_compress_wave_redo_kernel", "lz4_compress_wave_dict_kernel",
                        "lz4_compress_wave_dict_redo_kernel", "lz4_compress_wave_shared_kernel", "lz4_compress_wave_shared_redo_kernel"}, got
    assert all(int(v) <= 80 for v in got.values()), got
