"""The selection cases of tests/_selection_cases.py hold what they claim, from the oracle alone (no device): the listed
slots tie exactly at the strict minimum and the oracle returns the lowest of them; NaN, infinite and finite sums are
where the case says.  A case whose precondition fails would let tests/test_gpu_selection.py pass without deciding
anything, so it fails here; none is skipped."""
import numpy as np
import pytest

import _selection_cases as SC


@pytest.mark.parametrize("name", SC.NAMES)
def test_case_precondition(oracle, golden, name):
    case = SC.CASES[SC.NAMES.index(name)]
    ped, p0 = golden["sparse"], golden["r_p0uu"]
    assert ped.shape[0] == 78
    built = SC.build(case, oracle, ped, p0)
    assert built["models"].shape == (case["S"], 4)
    SC.check_precondition(case, built)


def test_cases_cover_the_kernel_s_paths():
    """the per-lane loop's later trips, both orders of a cross-lane tie, a same-lane tie, lanes without a candidate"""
    ties = [c for c in SC.CASES if c["slots"] is not None and len(c["slots"]) > 1]
    assert len(SC.NAMES) == len(set(SC.NAMES)) == len(SC.TIES) + len(SC.SPECIAL)
    assert max(c["S"] for c in SC.CASES) == 1000 and min(c["S"] for c in SC.CASES) == 1
    lanes = [[s % SC.WAVE for s in c["slots"]] for c in ties]
    low_lane_of_winner = [(min(c["slots"]) % SC.WAVE, [s % SC.WAVE for s in c["slots"] if s != min(c["slots"])]) for c in ties]
    assert any(len(set(ln)) < len(ln) for ln in lanes)                       # two tied slots in one lane
    assert any(w > min(o) for w, o in low_lane_of_winner)                    # the winner sits in the HIGHER lane
    assert any(w < min(o) for w, o in low_lane_of_winner)                    # ... and in the lower one
    assert any(c["winner"] is not None and c["winner"] >= SC.WAVE for c in SC.CASES)
    whole_lane = [c for c in SC.SPECIAL if c["nan"] and {s for s in range(c["S"]) if s % SC.WAVE == 7} <= set(c["nan"])]
    assert whole_lane                                                        # a lane all of whose starts are NaN


def test_tie_construction_keeps_every_other_sum(oracle, golden):
    """with_minimum_at changes the listed slots and the old winner's slot, nothing else"""
    ped, p0 = golden["sparse"], golden["r_p0uu"]
    base = SC.base_models(5, 70)
    k = oracle.select_best(ped, p0, base)[0]
    slots = tuple(s for s in (66, 3) if s != k)
    got = SC.with_minimum_at(oracle, ped, p0, base, slots)
    changed = np.flatnonzero(np.any(got != base, axis=1))
    assert set(changed) <= set(slots) | {k}
    assert all(np.array_equal(got[s], base[k]) for s in slots) and np.array_equal(got[k], base[slots[0]])
