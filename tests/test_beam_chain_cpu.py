"""The chain helper (tests/beam_chain.py) without a GPU: `run_chain` accepts an emulation of mm_beam_step built from beam_ref and
flags three deliberately wrong ones; the near counts and coverage flags of every chain case on the CPU (beam_ref evolving its own fp64
state) are recorded here as assertions, and tests/test_beam_chain_contract_gpu.py holds the library to the same flags."""
import pytest
import torch

from tests import beam_chain as BC

_pred = {}


def predicted(c):
    if c["name"] not in _pred:
        _pred[c["name"]] = BC.predict(c)
    return _pred[c["name"]]


@pytest.mark.parametrize("c", BC.CASES, ids=[c["name"] for c in BC.CASES])
def test_cpu_near_counts_and_coverage(c):
    seen = predicted(c)
    print(f"{c['name']}: {seen.pairs} (step, prompt) pairs, near {seen.near}, flags {seen.flags}")
    assert seen.pairs == c["T"] * c["B"]
    assert len(seen.near) == c["expect"]["near"], seen.near
    seen.check(c["expect"]["flags"])


def test_the_cases_cover_what_the_issue_lists():
    flags = {c["name"]: c["expect"]["flags"] for c in BC.CASES}
    assert {(c["n"], c["B"], c["V"], c["T"], c["es"], c["lp"]) for c in BC.CASES} == {
        (16, 2, 1003, 20, False, 1.0), (5, 3, 1003, 120, "never", 1.0), (2, 2, 64, 300, False, 1.0), (3, 2, 64, 270, True, 0.0),
        (16, 1, 4097, 20, False, 1.0)}
    assert BC.by_name("n16-V4097")["dtype"] == torch.float32
    assert flags["n16-T20"]["copy_trips"] >= 2                                      # step * n > 256
    assert flags["n5-T120"]["copy_trips"] >= 3 and flags["n5-T120"]["ragged_tail"] and flags["n5-T120"]["replaced_worst"]
    assert flags["n2-T300"]["empty_until_last"] and flags["n2-T300"]["all_enter_last"] and flags["n2-T300"]["entered_len_over_256"]
    assert flags["n3-T270"]["entered_len_over_256_before_last"] and flags["n3-T270"]["full_es_stepped"]
    assert flags["n16-V4097"]["short_chunk_won"]
    assert any(f.get("closed_stepped") for f in flags.values())


# every case against the right emulation; the wrong ones where their mistake can show
@pytest.mark.parametrize("c", BC.CASES, ids=[c["name"] for c in BC.CASES])
def test_run_chain_accepts_the_emulation(c):
    seen, xs, digests = BC.run_chain(BC.Emulation(c), c)
    print(f"{c['name']}: near {seen.near} of {seen.pairs}")
    seen.check(c["expect"]["flags"])                                               # the flags, and the 10 % cap on what was seen
    _, _, again = BC.run_chain(BC.Emulation(c), c, xs=xs)
    assert again == digests


@pytest.mark.parametrize("name,fault,match", [
    ("n16-T20", "anc256", "table entry outside|table spells another sequence"),
    ("n5-T120", "anc256", "table entry outside|table spells another sequence"),
    ("n2-T300", "fseq255", "no running sequence plus a stopping token"),
    ("n3-T270", "fseq255", "no running sequence plus a stopping token"),
    ("n16-V4097", "zero-keys", None),
])
def test_run_chain_flags_a_wrong_step(name, fault, match):
    c = BC.by_name(name)
    with pytest.raises(AssertionError, match=match):
        BC.run_chain(BC.Emulation(c, fault), c)


def test_single_step_cases_on_the_cpu():
    """the cases of tests/test_beam_step_contract_gpu.py need no GPU to be built: their list covers what it must, the planted ties
    and maxima sit where the cases want them (asserted by build), and at most a tenth of them is near"""
    from tests import test_beam_step_contract_gpu as S
    S.test_the_cases_cover_what_the_issue_lists()
    ids = [S.case_id(c) for c in S.CASES]
    assert len(set(ids)) == len(ids)
    near = [S.case_id(c) for c in S.CASES if S.build(c)["near"]]
    print(f"near: {len(near)} of {len(S.CASES)}: {near}")
    assert len(near) <= len(S.CASES) // 10, near
    assert not any(S.build(c)["near"] for c in S.CASES if c["ties"] or c["oob"] or c["off"] or (0 < c["V"] % 4096 < 2 * c["n"]))


def test_tau_grows_with_the_scores_only():
    assert BC.tau_for(0.0) == BC.tau_for(BC.SMAX) == BC.TAU and BC.tau_for(BC.SMAX + 500.0) == BC.TAU + 1000.0 * BC.U32
