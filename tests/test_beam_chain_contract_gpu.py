"""mm_beam_step chained on its own state: K.beam_step for i = 0 .. T-1 on one K.BeamState, never stopping at `done`, then
mm_beam_finish -- through tests/beam_chain.run_chain (the teacher-forced fp64 reference, the host mirror of the sequences, the frozen
finished sets; tests/test_beam_chain_cpu.py shows which wrong kernels it flags).  The single steps of
tests/test_beam_step_contract_gpu.py run on states the test wrote and never beyond 8 tokens; here the ping-pong tables, the slots and
arrival numbers are the kernel's own, and the strided copy loops of beam_merge_kernel and beam_finish_kernel take a second, third and
ragged trip.

Every case asserts the coverage flags recorded beside it (tests/beam_chain.CASES; the CPU's counts are asserted in
tests/test_beam_chain_cpu.py) and that at most 10 % of its (step, prompt) pairs were near; it prints what it saw.  A second whole run
from a fresh state must write the same bits at every step."""
import pytest
import torch

from multimeditron_amd import kernels as K
from tests import beam_chain as BC

pytestmark = pytest.mark.gpu


class Library:
    """the device of run_chain: one K.BeamState; logits with a padded row stride and NaN in the padding"""

    def __init__(self, c, pad=5):
        self.c, self.pad = c, pad

    def reset(self):
        c = self.c
        self.st = K.BeamState(c["B"], c["n"], c["T"], c["V"], "cuda")
        self.st.buf.fill_(0x7F)                                                     # nothing needs clearing: junk everywhere
        self.st.next_ids.fill_(-1)

    def step(self, x, i):
        c = self.c
        wide = torch.full((x.shape[0], c["V"] + self.pad), float("nan"), dtype=c["dtype"])
        wide[:, :c["V"]] = x
        K.beam_step(wide.cuda()[:, :c["V"]], self.st, i, c["eos"], c["lp"], c["es"])

    def fields(self):
        torch.cuda.synchronize()
        return {name: getattr(self.st, name).cpu().clone() for name in BC.FIELDS}

    def finish(self, nrs):
        return tuple(t.cpu() for t in K.beam_finish(self.st, nrs, self.c["eos"]))


@pytest.mark.parametrize("c", BC.CASES, ids=[c["name"] for c in BC.CASES])
def test_beam_chain_contract(c):
    seen, xs, digests = BC.run_chain(Library(c), c)
    print(f"{c['name']}: {c['T']} steps, {seen.pairs} (step, prompt) pairs, near on the GPU {seen.near} (CPU prediction: "
          f"{c['expect']['near']}), worst |score - ref| / lp_bound = {seen.ratio[0]:.3f} at step {seen.ratio[1]}, flags {seen.flags}")
    seen.check(c["expect"]["flags"])                                               # every reason of the case occurred; the 10 % cap
    _, _, again = BC.run_chain(Library(c), c, xs=xs)
    assert again == digests, [i for i, (a, b) in enumerate(zip(again, digests)) if a != b][:5]
