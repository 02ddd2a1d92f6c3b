"""Two training passes of every tiny model: the launches and the gradient-ready calls, by name and in order, against
tests/golden/train_launches.jsonl.

The gradient tests would still pass if an autograd Function swapped two launches that do not depend on each other, queued one more,
or announced a parameter's gradient before the launch that writes it.  The file was recorded, with tests/train_trace.py's record()
(`python tools/make_golden.py train_launches`), from the autograd layer as it stood before its projection backward, its gradient
write and its q|k|v split each became one function; the same record() must reproduce it.  The second pass of every case
accumulates into the gradients of the first.  Names only; nothing is timed."""
import pytest
import torch

from tests import train_trace as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def want(golden_dir):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    rows = T.read(golden_dir)
    assert [c for c, _ in rows] == T.NAMES
    return dict(rows)


@pytest.mark.parametrize("case", T.NAMES)
def test_training_queues_the_recorded_launches(want, golden_dir, tmp_path, case):
    w = want[case]
    with T.switches(case):
        params, step = T.build_case(case, golden_dir, tmp_path)
        g = T.recorded(params, step)
    print(f"{case}: {len(g)} entries, {sum(n.startswith('ready:') for n in g)} ready (recorded: {len(w)})")
    if g != w:
        at = next((i for i, (x, y) in enumerate(zip(g, w)) if x != y), min(len(g), len(w)))
        pytest.fail(f"{case}: first difference at entry {at}: got {g[at:at + 4]} want {w[at:at + 4]} ({len(g)} against {len(w)} entries)")
