"""Early bootstraps (abn_plan_run): on a one-window plan phase B is launched once a quorum of the starts has
finished; the stragglers finish beside it, and phase B is stopped and redone when one of them turns out best.  A gamble in
time only: every byte of every output is what the plan computes with early bootstraps off, and what the oracle computes.

All on the C3 topology (105 rows), S = 10 starts, quorum 8.  Every case first derives from the oracle which start is best
and in which order the starts finish (iterations; a stuck fit ends at once on the device: the fixed-point skip) and asserts
the precondition it is about, so that none can pass vacuously."""
import numpy as np
import pytest

from alphabeta_rs_amd import synthetic

import _parity

# B: the fewest bootstraps (a multiple of four and some) that the route gives to the persistent kernel on this topology — four
# chains per wavefront, more than 2048 wavefronts; up to 8192 bootstraps run on the plain resident kernel and such a plan
# is not eligible (test_ineligible_plans_run_as_before has one)
SEED, S, B, QUORUM = 20260101, 10, 8200, 8
ITERS_A, ITERS_B = 10000, 1000
KEYS = ("models", "pred", "resid", "raw", "best_start")
pytestmark = pytest.mark.gpu


def window_case(which):
    """(pedigree N x 4, p0uu, window_offset): the C3 benchmark window, or window `which` of the C4 set"""
    if which == "c3":
        ped, p0 = synthetic.c3_pedigree()
        return ped, p0, 0
    gens, D, p0, _ = synthetic.c4_windows(1, window_offset=which)
    return np.concatenate([gens, D[0][:, None]], axis=1), float(p0[0]), which


@pytest.fixture(scope="module")
def reference(abn, oracle):
    """per case, computed once and never changed: the oracle's fits of the ten starts, the selection over them, the best
    start, the starts in finishing order and 64 sampled bootstrap rows"""
    cache = {}

    def get(which):
        if which not in cache:
            ped, p0, woff = window_case(which)
            tree = abn.reduction_tree(ped[:, :3], abn.default_options(seed=SEED))
            s0 = abn.gen_start_simplices(SEED, woff, S, float(ped[:, 3].max()))
            fits = oracle.fit_batch(ped, p0, p0, 1.0, s0, ITERS_A, lanes=tree)
            best, model, pred, resid, _ = oracle.select_best(ped, p0, fits["best"])
            length = np.where((fits["status"] == 1) & (fits["iters"] == ITERS_A), 0, fits["iters"])  # stuck: ends at once
            order = np.argsort(length, kind="stable")
            rows = np.random.default_rng(7).choice(B, 64, replace=False)
            boot = [oracle.boot_model(ped, model, pred, resid, p0, p0, 1.0, SEED, woff, int(b), 1, max_iters=ITERS_B,
                                      lanes=tree, threads=4) for b in rows]
            cache[which] = dict(ped=ped, p0=p0, woff=woff, fits=fits, best=int(best), model=model, pred=pred, resid=resid,
                                length=length, order=order, rows=rows, boot=boot)
        return cache[which]

    return get


def make_plan(abn, ctx, ref, mode, n_boot=B, **options):
    plan = abn.Plan(ctx, ref["ped"][:, :3], 1, S, n_boot, window_offset=ref["woff"], options=abn.default_options(seed=SEED, **options))
    plan.set_early_bootstraps(mode)
    plan.set_windows(ref["ped"][:, 3][None, :], np.array([ref["p0"]]))
    return plan


def run_once(abn, ctx, ref, mode, **kw):
    """(download(), early_bootstraps(), counters(), tail_handed(), last_kernels()) of one run of a fresh plan"""
    plan = make_plan(abn, ctx, ref, mode, **kw)
    plan.run()
    res = plan.download(), plan.early_bootstraps(), plan.counters(), plan.tail_handed(), plan.last_kernels()
    plan.close()
    return res


def assert_same_bytes(a, b, label=None):
    for k in KEYS + ("info_a", "info_b"):
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), (label, k)


def assert_oracle(out, ref, label=None):
    """starts, selection and the 64 sampled bootstrap rows, byte for byte"""
    _parity.assert_fits_equal(None, out["info_a"][0], ref["fits"], label)
    assert out["best_start"][0] == ref["best"] and np.array_equal(out["models"][0], ref["model"]), label
    assert np.array_equal(out["pred"][0], ref["pred"]) and np.array_equal(out["resid"][0], ref["resid"]), label
    for b, (raw, res) in zip(ref["rows"], ref["boot"]):
        assert np.array_equal(out["raw"][0, b:b + 1], raw, equal_nan=True), (label, b)
        for f in ("iters", "evals", "status"):
            assert np.array_equal(out["info_b"][f][0, b:b + 1], res[f]), (label, b, f)


def test_hit_is_byte_equal_to_the_late_launch_and_the_oracle(abn, gpu_ctx, reference):
    """(a) C3: the best start is among the first eight finishers and the two longest chains are far behind the eighth"""
    ref = reference("c3")
    first8, last2 = ref["order"][:QUORUM], ref["order"][QUORUM:]
    assert ref["best"] in first8, (ref["best"], ref["order"], ref["length"])
    assert ref["length"][last2].min() > 1.2 * ref["length"][first8].max(), ref["length"]   # 645 and 893 against 512
    off, st0, cnt0, _, _ = run_once(abn, gpu_ctx, ref, 0)
    on, st1, cnt1, handed, kinds = run_once(abn, gpu_ctx, ref, 1)
    assert kinds["starts"][0] == "speculative" and kinds["boot"][0] == "persistent", kinds
    assert st0 == {"eligible": True, "quorum": QUORUM, "parked": 0, "miss": False}, st0      # off: nothing parked
    assert st1 == {"eligible": True, "quorum": QUORUM, "parked": S - QUORUM, "miss": False}, st1
    assert_same_bytes(on, off)
    assert cnt1 == cnt0 and handed[1] > 0, (cnt0, cnt1, handed)
    assert_oracle(on, ref)


@pytest.mark.parametrize("window", (4, 22))
def test_miss_redoes_the_bootstraps(abn, gpu_ctx, reference, window):
    """(b) the best start is the longest chain (1139 against 1070 iterations, 1041 against 933): phase B, launched on a
    model that does not stand, is stopped and redone; the counters are those of one complete phase B"""
    ref = reference(window)
    assert ref["best"] == ref["order"][-1] and ref["length"][ref["best"]] > ref["length"][ref["order"][-2]], \
        (ref["best"], ref["order"], ref["length"])
    off, _, cnt0, handed0, _ = run_once(abn, gpu_ctx, ref, 0)
    on, st1, cnt1, handed1, kinds = run_once(abn, gpu_ctx, ref, 1)
    assert kinds["starts"][0] == "speculative" and kinds["boot"][0] == "persistent", kinds
    assert st1["eligible"] and st1["quorum"] == QUORUM and st1["miss"] and 1 <= st1["parked"] <= S - QUORUM, st1
    assert_same_bytes(on, off, window)
    assert_oracle(on, ref, window)
    assert cnt1 == cnt0, (cnt0, cnt1)                       # fits, evaluations, iterations, skipped: one phase A, one phase B
    assert handed0[0] == handed1[0] == 0 and 0 < handed1[1] <= 1024 and 0 < handed0[1] <= 1024, (handed0, handed1)


def test_stale_state_of_an_earlier_window_never_shows(abn, gpu_ctx, reference):
    """(c) run on window X (window 4, a miss: parked rows, a raised miss word, a stopped table), set_windows to Y (the C3
    observations in the same plan, so under window 4's random streams), run again: the bytes and the statistics of a fresh
    plan on Y"""
    x, y = reference(4), reference("c3")
    assert x["best"] == x["order"][-1]

    def plan_on(first):
        plan = abn.Plan(gpu_ctx, x["ped"][:, :3], 1, S, B, window_offset=x["woff"], options=abn.default_options(seed=SEED))
        stats = []
        for ref in first:
            plan.set_windows(ref["ped"][:, 3][None, :], np.array([ref["p0"]]))
            plan.run()
            stats.append(plan.early_bootstraps())
        out = plan.download()
        plan.close()
        return out, stats

    fresh, st_fresh = plan_on([y])
    out, st = plan_on([x, y])
    assert st[0]["miss"] and st[1] == st_fresh[0] and st[1]["eligible"], (st, st_fresh)
    assert_same_bytes(out, fresh)


@pytest.mark.parametrize("case", ("windows", "few_bootstraps", "strict_order"))
def test_ineligible_plans_run_as_before(abn, gpu_ctx, case):
    """(d) three windows, 500 bootstraps (phase B on the speculative kernel) and strict order: not eligible, same bytes"""
    W, nb, opts = (3, B, {}) if case == "windows" else (1, 500, {}) if case == "few_bootstraps" else (1, B, {"strict_order": 1})
    gens, D, p0, _ = synthetic.c4_windows(W, window_offset=4)
    outs = []
    for mode in (0, 1):
        plan = abn.Plan(gpu_ctx, gens, W, S, nb, window_offset=4, options=abn.default_options(seed=SEED, **opts))
        plan.set_early_bootstraps(mode)
        plan.set_windows(D, p0)
        plan.run()
        outs.append(plan.download())
        st = plan.early_bootstraps()
        plan.close()
        assert st == {"eligible": False, "quorum": 0, "parked": 0, "miss": False}, (case, mode, st)
    assert_same_bytes(outs[0], outs[1], case)


@pytest.mark.parametrize("which", ("c3", 22))
def test_ten_runs_without_a_sync_are_one_run(abn, gpu_ctx, reference, which):
    """(e) back to back on the stream (a hit, a miss): every counter and flag of a run is cleared by the next"""
    ref = reference(which)
    one, st_one, cnt_one, _, _ = run_once(abn, gpu_ctx, ref, 1)
    plan = make_plan(abn, gpu_ctx, ref, 1)
    for _ in range(10):
        plan.run()
    out, st, cnt = plan.download(), plan.early_bootstraps(), plan.counters()
    plan.close()
    assert st == st_one and cnt == cnt_one and st["miss"] == (which != "c3"), (st, st_one, cnt, cnt_one)
    assert_same_bytes(out, one, which)
    assert_oracle(out, ref, which)
