"""The selection on the device (abn_select_lse_kernel, abn_select_kernel; src/ab_neutral.rs:83-135) against the oracle's
abo_select_best on identical inputs, bit for bit (two NaN count as equal): the cases of tests/_selection_cases.py — ties
at the minimum within a lane and across lanes, up to 1000 starts, NaN and infinite sums — whose preconditions
tests/test_selection_cases_cpu.py asserts from the oracle alone; row counts at the edges of the serial sum's 512-term
chunk; inputs without any finite fit; and the selection inside a plan of 130 starts per window."""
import numpy as np
import pytest

import _selection_cases as SC
from _parity import assert_same_bits, synthetic_pedigree

pytestmark = pytest.mark.gpu

NO_FINITE_FIT = 5


def _compare(got, want, label):
    k, model, pred, resid, lse = got
    wk, wmodel, wpred, wresid, wlse = want
    assert k == wk, (label, k, wk)
    assert_same_bits(lse, wlse, f"{label}: lse")
    assert_same_bits(model, wmodel, f"{label}: model")
    assert_same_bits(pred, wpred, f"{label}: pred")
    assert_same_bits(resid, wresid, f"{label}: resid")


@pytest.mark.parametrize("name", SC.NAMES)
def test_select_best_case(gpu_ctx, oracle, golden, name):
    case = SC.CASES[SC.NAMES.index(name)]
    ped, p0 = golden["sparse"], golden["r_p0uu"]
    built = SC.build(case, oracle, ped, p0)
    SC.check_precondition(case, built)
    got = gpu_ctx.select_best(ped, p0, built["models"])
    if case["winner"] is not None:
        assert got[0] == case["winner"], (name, got[0])
    _compare(got, built["want"], name)


@pytest.mark.parametrize("n", (1, 63, 64, 65, 511, 512, 513, 1024, 1025))
def test_serial_sum_at_the_chunk_edges(gpu_ctx, oracle, n):
    """kSelChunk = 512 terms go through LDS at a time and are added serially in row order: the order is the result.  Three
    random models and a copy of the best of them in the last slot: the tie is at the minimum, the lower index wins."""
    ped = synthetic_pedigree(np.random.default_rng(4000 + n), n, 12)
    p0 = 0.8
    base = SC.base_models(5000 + n, 3)
    k = oracle.select_best(ped, p0, base)[0]
    models = np.vstack([base, base[k]])
    want = oracle.select_best(ped, p0, models)
    wlse = want[4]
    assert want[0] == k and wlse[3].view(np.uint64) == wlse[k].view(np.uint64)
    assert np.all(np.delete(wlse, [k, 3]) > wlse[k])
    _compare(gpu_ctx.select_best(ped, p0, models), want, f"N={n}")


@pytest.mark.parametrize("S", (1, 130))
def test_no_finite_fit_is_a_status(abn, gpu_ctx, oracle, golden, S):
    ped, p0 = golden["sparse"], golden["r_p0uu"]
    models = np.full((S, 4), np.nan)
    assert oracle.select_best(ped, p0, models)[0] == -1
    with pytest.raises(abn.AbnError) as e:
        gpu_ctx.select_best(ped, p0, models)
    assert e.value.status == NO_FINITE_FIT


# seed 10 of the plan below: the oracle's winners are the starts 124, 75 and 71, all in the second trip of their lanes (60, 11
# and 7); found with the oracle alone, asserted below
PLAN_SEED = 10


def test_selection_inside_a_plan_past_64_starts(abn, gpu_ctx, oracle, golden):
    """the bundled six-row pedigree, W = 3, S = 130, B = 2: abn_select_kernel's per-lane loop takes a second and a third
    trip inside abn_plan_run, and what it selects is what the bootstraps run on"""
    ped, p0 = golden["generated"], golden["p0uu_generated"]
    W, S, B, ia, ib = 3, 130, 2, 30, 10
    rng = np.random.default_rng(23)
    D = np.tile(ped[:, 3], (W, 1))
    D[1:] = np.abs(D[1:] * rng.uniform(0.7, 1.3, (W - 1, 1)))
    o = abn.default_options(seed=PLAN_SEED, max_iters_start=ia, max_iters_boot=ib)
    plan = abn.Plan(gpu_ctx, ped[:, :3], W, S, B, options=o)
    plan.set_windows(D, np.full(W, p0))
    plan.run()
    out = plan.download()
    plan.close()
    tree = abn.reduction_tree(ped[:, :3], o)
    assert np.all(out["info_a"]["lanes"] == tree) and np.all(out["info_b"]["lanes"] == tree)
    winners = []
    for w in range(W):
        pw = np.concatenate([ped[:, :3], D[w][:, None]], axis=1)
        s0 = abn.gen_start_simplices(PLAN_SEED, w, S, D[w].max())
        fits = oracle.fit_batch(pw, p0, p0, 1.0, s0, ia, lanes=tree, threads=4)
        for f in ("status", "iters", "evals"):
            assert np.array_equal(out["info_a"][f][w], fits[f]), (w, f)
        k, model, pred, resid, _ = oracle.select_best(pw, p0, fits["best"])
        winners.append(k)
        assert out["best_start"][w] == k, (w, out["best_start"][w], k)
        assert_same_bits(out["models"][w], model, f"window {w}: model")
        assert_same_bits(out["pred"][w], pred, f"window {w}: pred")
        assert_same_bits(out["resid"][w], resid, f"window {w}: resid")
        wraw, _ = oracle.boot_model(pw, model, pred, resid, p0, p0, 1.0, PLAN_SEED, w, 0, B, max_iters=ib, lanes=tree)
        assert_same_bits(out["raw"][w], wraw, f"window {w}: raw")
    assert winners == [124, 75, 71] and max(winners) >= 64, winners
