"""The streams of the paged tests (tests/test_paged_model.py on the CPU, tests/test_gpu_paged.py on the GPU): lengths around every edge of
the rule for a page size P, an incompressible stream that meets the page bound exactly, a run of zeros that retries up to window_max,
and text and JSON.  A plain module, not a fixture."""
import corpus
import oracle_api as O
import paged_model as M

PAGE_SIZES = [64, 509, 4096]


def streams(page_size, cut=20 * 1024, zeros=64 * 1024):
    """[(name, bytes)]: `cut` = the length the text and JSON fixtures are cut to, `zeros` = the length of the zero stream"""
    L = M.lfit_page(page_size)
    text = O.fixture_plain("compression_34k")[:cut]
    json = O.fixture_plain("compression_66k_JSON")[:cut]
    out = [("len%d" % k, text[:k]) for k in (0, 1, 5, 12, 13, 63, 64, 65)]
    out += [("lfit", corpus.lcg_bytes(L, 7)), ("lfit+1", corpus.lcg_bytes(L + 1, 9))]      # one page of literals, and one byte more
    out.append(("noise", corpus.lcg_bytes(3 * page_size + 7, 41)))
    out.append(("zeros", bytes(zeros)))
    out += [("text", text), ("json", json)]
    return out
