"""generate()'s launches, by name and in order, against tests/golden/generate_launches.jsonl.

The bit tests of generate (test_generate_{samples,beams,processors,lookup}_gpu, test_sampling_gpu, test_model_gpu) would still pass if
the decode loop swapped two launches that do not depend on each other, queued one more, or looked at its done flag at another cadence.
The file was recorded, with tests/generate_trace.py's record() (`python tools/make_golden.py generate_launches`), from the three
separate loops that stood behind generate() before they became one driver with three strategies; the same record() must reproduce
it: every mode of generate on the d128 fixture for 4 tokens, and for each strategy one run that ends early, whose number of decoder
passes shows at which steps the host looked.  Names only; nothing is timed."""
import pytest

from tests import generate_trace as T

pytestmark = pytest.mark.gpu


def test_generate_queues_the_recorded_launches(golden_dir, tmp_path):
    want = T.read(golden_dir)
    assert [c for c, _ in want] == [c for c, _ in T.CASES + T.EARLY]
    got = T.record(*T.load(golden_dir, tmp_path))
    bad = []
    for (case, g), (_, w) in zip(got, want):
        print(f"{case}: {len(g)} launches, {g.count('mm_embed_splice_fwd')} decoder passes (recorded: {len(w)}, {w.count('mm_embed_splice_fwd')})")
        if g != w:
            at = next((i for i, (x, y) in enumerate(zip(g, w)) if x != y), min(len(g), len(w)))
            bad.append(f"{case}: first difference at launch {at}: got {g[at:at + 4]} want {w[at:at + 4]} ({len(g)} against {len(w)} launches)")
    assert not bad, "\n".join(bad)
