"""Every inference route of CausalLM.forward queues the launches of tests/golden/decoder_routes.jsonl, by name and in order.

The table was recorded once, by tests/decoder_routes.record() (`python tools/make_golden.py decoder_routes`), on the revision whose
routes are the contract; here the same recorder runs on this tree, without a GPU (it launches nothing: see tests/decoder_routes.py).
It pins what the bit tests cannot see -- a route that quietly took the separate launches instead of the fused ones, the generic
linear instead of the weight-streaming one, or another cache's attention -- for the full product of families, MM_DECODE_FUSED, caches
and weight formats, the refused combinations included (their exception text is the entry)."""
import itertools
import os

import pytest

from tests import decoder_routes as T

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def want():
    return dict(T.read(GOLDEN))


@pytest.fixture(scope="module")
def got():
    return dict(T.record())


def test_the_table_holds_the_full_product_of_cases():
    """the cap: no case can leave the table (or the recorder's list) unnoticed"""
    ids = [name for name, _ in T.read(GOLDEN)]
    product = ["-".join((f, "fused" if x == "1" else "separate", c, w))
               for f, x, c, w in itertools.product(("llama", "qwen2", "qwen3", "apertus"), ("1", "0"),
                                                   ("plain", "kv8", "samples3", "beams3", "lookup3", "lookup3-S1", "rows17", "fp32"),
                                                   ("bf16", "dw", "dw+pw"))]
    wide = ["-".join(("llama-wide", x, c, w)) for x in ("fused", "separate") for c in ("lookup3-B4", "lookup3-B2") for w in ("bf16", "dw")]
    assert ids == product + wide and len(ids) == 192 + 8
    assert ids == [T.case_id(c) for c in T.CASES]


def test_the_wide_verify_places_down_proj_by_its_rows(want):
    """16 rows of 4608 features exceed the weight-streaming kernel's LDS stage (fused down_proj is mm_gemm), 8 rows fit it"""
    assert want["llama-wide-fused-lookup3-B4-bf16"]["step"][-2:] == ["mm_gemm", "mm_decode_linear"]           # down_proj, norm + lm_head
    assert want["llama-wide-fused-lookup3-B2-bf16"]["step"][-2:] == ["mm_decode_linear", "mm_decode_linear"]
    assert "mm_rmsnorm_fwd" not in want["llama-wide-fused-lookup3-B4-bf16"]["step"]


@pytest.mark.parametrize("name", [T.case_id(c) for c in T.CASES])
def test_route(name, got, want):
    assert got[name] == want[name], "\n".join(f"{k}:\n  got  {got[name].get(k)}\n  want {want[name].get(k)}" for k in want[name])
