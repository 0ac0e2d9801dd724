"""Inputs of the selection (abn_select_lse_kernel, abn_select_kernel: src/ab_neutral.rs:83-135) whose answer hangs on the
tie rule, on a start past the 64th, or on NaN / infinite sums: plain data and host arithmetic, no device.

tests/test_selection_cases_cpu.py asserts every case's precondition from the oracle alone — the listed slots hold the
strict minimum, NaN and infinite sums are where the case says — and tests/test_gpu_selection.py runs the same cases on the
device.  abn_select_kernel gives lane l the starts l, l + 64, ... and folds the 64 candidates with a butterfly: the slots
below are named by the lane (slot % 64) and the trip (slot // 64) they fall on.

A tie is made constructively: the oracle's sums over the base models, the arg-min model m* copied into the listed slots,
and the model the first of them held moved to where m* was (when that is not a listed slot).  Every other sum is one of the
base models', so strictly larger unless two random models happen to tie, which the CPU test would report.
"""
import numpy as np

WAVE = 64
BASE = np.array([5.8e-05, 6.5e-03, 0.03, 6e-05])
INF_INTERCEPT = 1e200        # (D - 1e200 - dt)^2 overflows: every term, hence the sum, is +inf


def base_models(seed, S):
    return BASE * np.random.default_rng(seed).uniform(0.5, 1.5, (S, 4))


def with_minimum_at(oracle, ped, p0, base, slots):
    """`base` with its arg-min model (the oracle's sums) in every slot of `slots` and nowhere else"""
    models = np.array(base, dtype=np.float64)
    k, _, _, _, _ = oracle.select_best(ped, p0, models)
    assert k >= 0
    best = models[k].copy()
    if k not in slots:
        models[k] = models[slots[0]]
    for s in slots:
        models[s] = best
    return models


# (S, slots holding the minimum): what the tie decides
TIES = (
    (9, (3, 7)),                  # one trip, two lanes
    (64, (62, 63)),               # the last two lanes of a full single trip
    (65, (0, 64)),                # the same lane, trips 0 and 1: the per-lane loop keeps the first
    (65, (63, 64)),               # the lower index in lane 63, the higher in lane 0: the fold prefers the index, not the lane
    (128, (5, 69, 70)),           # lane 5 twice (kept: 5), lane 6 once
    (129, (127, 128)),            # lane 63 trip 1 against lane 0 trip 2
    (1000, (370, 371, 999)),      # the size the kernel's comment quotes; 999 is the last start
    (1000, (936, 64)),            # the lower index is listed last: lane 0 trip 1 against lane 40 trip 14
    (130, (129,)),                # no tie: the unique minimum is the last start of a partly filled third trip
    (1, (0,)),                    # S = 1
)

# cases without ties: NaN sums (alpha = NaN) and +inf sums (intercept 1e200).  S = 200: lane 7 holds 7, 71, 135 and 199.
SPECIAL = (
    dict(name="nan_slot0_and_lane7", S=200, nan=(0, 7, 71, 135), inf=(), winner=None),
    dict(name="nan_slot0_and_all_of_lane7", S=200, nan=(0, 7, 71, 135, 199), inf=(), winner=None),
    dict(name="all_inf", S=70, nan=(), inf=tuple(range(70)), winner=0),
    dict(name="inf_but_slot69", S=70, nan=(), inf=tuple(s for s in range(70) if s != 69), winner=69),
    dict(name="nan_first_trip_finite_slot64", S=65, nan=tuple(range(64)), inf=(), winner=64),
)


def _tie_name(S, slots):
    return f"S{S}_min_at_" + "_".join(str(s) for s in slots)


CASES = tuple(dict(name=_tie_name(S, slots), S=S, slots=slots, nan=(), inf=(), winner=min(slots), seed=1000 + i)
              for i, (S, slots) in enumerate(TIES)) + \
    tuple(dict(c, slots=None, seed=2000 + i) for i, c in enumerate(SPECIAL))
NAMES = tuple(c["name"] for c in CASES)

_built = {}


def build(case, oracle, ped, p0):
    """{"models": (S, 4), "want": the oracle's (index, model, pred, resid, lse)} of one case, built once per process"""
    if case["name"] not in _built:
        models = base_models(case["seed"], case["S"])
        if case["slots"] is not None:
            models = with_minimum_at(oracle, ped, p0, models, case["slots"])
        for s in case["nan"]:
            models[s, 0] = np.nan
        for s in case["inf"]:
            models[s, 3] = INF_INTERCEPT
        models.setflags(write=False)
        _built[case["name"]] = {"models": models, "want": oracle.select_best(ped, p0, models)}
    return _built[case["name"]]


def check_precondition(case, built):
    """what the case is for, from the oracle's sums alone"""
    k, _, _, _, lse = built["want"]
    S = case["S"]
    assert lse.shape == (S,)
    nan, inf = np.zeros(S, bool), np.zeros(S, bool)
    nan[list(case["nan"])] = True
    inf[list(case["inf"])] = True
    assert np.array_equal(np.isnan(lse), nan), case["name"]
    assert np.array_equal(np.isposinf(lse), inf), case["name"]
    finite = np.isfinite(lse)
    assert np.array_equal(finite, ~(nan | inf)), case["name"]
    if case["slots"] is not None:
        slots = list(case["slots"])
        low = lse[slots[0]]
        assert np.all(lse[slots].view(np.uint64) == low.view(np.uint64)), case["name"]      # an exact tie
        rest = np.ones(S, bool)
        rest[slots] = False
        assert np.all(lse[rest & finite] > low), case["name"]                                # ... at the strict minimum
        assert k == min(slots) == case["winner"], (case["name"], k)
    elif case["winner"] is not None:
        assert k == case["winner"], (case["name"], k)
    else:                     # the minimum is elsewhere: a finite slot, strictly below every other finite sum
        assert finite[k] and np.all(lse[finite & (np.arange(S) != k)] > lse[k]), (case["name"], k)
    if finite.any():
        assert finite[k], case["name"]
