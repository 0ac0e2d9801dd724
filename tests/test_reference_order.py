"""The reference sums a cost's residuals SERIALLY in row order (`square_sum += ...`, src/structs.rs:206-213); the product's
default sums them with the pedigree's canonical tree, so a cost differs in the last ulp and Nelder-Mead,
which branches on comparisons of nearly equal costs, may take another trajectory.  These tests measure what that does
to a whole fit — `ab_neutral::run` + `boot_model::run` on identical start simplices and bootstrap indices, the oracle's
lanes = 1 (reference order) beside the tree — and hold the north star's bar: the reported model and the predicted
divergences within 1e-6 of the reference-order run.  They also pin how many individual starts / bootstrap rows differ
by more than that (a start that reaches argmin's fixed point in one order and converges in the other differs by
O(1); it is never the selected one).  `strict_order = 1` removes the difference: the HIP fits are then bit-equal to
the oracle's lanes = 1 (GPU tests at the end).
"""
import numpy as np
import pytest

from _parity import synthetic_pedigree
from _route_model import CANON

SEED = 20260101
TOL = 1e-6   # north star: "within 1e-6 of the reference Rust" on alpha, beta, weight and the predicted divergence


def _cases(golden):
    from alphabeta_rs_amd import synthetic

    c3, c3_p0 = synthetic.c3_pedigree()
    return {
        # name: (pedigree, p0uu, starts, bootstraps, allowed beyond 1e-6: starts, bootstrap rows refitted from the SAME
        #        model, fraction of bootstrap rows of the whole pipeline)
        # measured (oracle, and the HIP path which is bit-equal to the oracle's tree order):
        #   generated: 2 / 1000 starts (they reach argmin's fixed point in one order and converge in the other: O(1)
        #              apart, never selected), 0 / 2000 rows from the same model (max 6.6e-7, in `weight`), 42 / 2000 rows
        #              end to end — the six-row pedigree does not identify `weight` (bootstrap SD 3.4), so the 4e-8
        #              between the two selected models, which moves every jittered start simplex, is amplified
        #   sparse, pedigree.txt, C3: every start and every row bit-identical
        "generated": (golden["generated"], golden["p0uu_generated"], 1000, 2000, 4, 2, 0.03),
        "sparse": (golden["sparse"], golden["r_p0uu"], 40, 200, 0, 0, 0.0),
        "pedigree": (golden["pedigree"], 0.75, 40, 200, 0, 0, 0.0),
        "c3": (c3, c3_p0, 40, 200, 0, 0, 0.0),
    }


def oracle_pipeline(O, ped, p0, S, B, lanes, window=0):
    """ab_neutral::run + boot_model::run with the deterministic inputs of the plan API (eqp = p0uu, weight 1)"""
    s0 = np.stack([O.start_simplex(SEED, window, s, ped[:, 3].max()) for s in range(S)])
    fits = O.fit_batch(ped, p0, p0, 1.0, s0, 10000, lanes=lanes)
    k, model, pred, resid, lse = O.select_best(ped, p0, fits["best"])
    raw, res = O.boot_model(ped, model, pred, resid, p0, p0, 1.0, SEED, window, 0, B, lanes=lanes)
    return {"fits": fits, "k": k, "model": model, "pred": pred, "resid": resid, "raw": raw, "res": res}


def compare(ref, got, raw_same_model, name, max_starts, max_rows, max_frac):
    """ref: reference order (lanes = 1); got: the product's order; raw_same_model: the product's bootstrap table when
    it is handed the reference-order run's model, predictions and residuals"""
    dm = np.abs(ref["model"] - got["model"]).max()
    dp = np.abs(ref["pred"] - got["pred"]).max()
    assert dm <= TOL and dp <= TOL, (name, dm, dp)
    ok = (ref["fits"]["status"] != 2) & (got["fits"]["status"] != 2)
    d_start = np.abs(ref["fits"]["best"] - got["fits"]["best"])[ok].max(axis=1)
    d_same = np.abs(ref["raw"] - raw_same_model).max(axis=1)
    d_row = np.abs(ref["raw"] - got["raw"]).max(axis=1)
    n_start, n_same, n_row = int((d_start > TOL).sum()), int((d_same > TOL).sum()), int((d_row > TOL).sum())
    other = int((ref["fits"]["evals"] != got["fits"]["evals"]).sum())
    print(f"{name}: selected model |d| {dm:.3g}, pred |d| {dp:.3g}; starts beyond 1e-6: {n_start}/{len(d_start)} "
          f"(max {d_start.max():.3g}; {other} on another trajectory); bootstrap rows beyond 1e-6: from the same model "
          f"{n_same}/{len(d_same)} (max {d_same.max():.3g}), end to end {n_row}/{len(d_row)} (max {d_row.max():.3g})")
    assert n_start <= max_starts, (name, n_start)
    assert n_same <= max_rows, (name, n_same, d_same.max())
    assert n_row <= max_frac * len(d_row), (name, n_row, d_row.max())
    # what the analysis reports (src/analysis.rs:50-98) is the same distribution: column means and SDs within 1 % of the SD
    sd_ref, sd_got = ref["raw"].std(axis=0, ddof=1), got["raw"].std(axis=0, ddof=1)
    assert np.all(np.abs(sd_ref - sd_got) <= 0.01 * sd_ref + 1e-15), (name, sd_ref, sd_got)
    assert np.all(np.abs(ref["raw"].mean(axis=0) - got["raw"].mean(axis=0)) <= 0.01 * sd_ref + 1e-15), name


@pytest.mark.parametrize("name", ["generated", "sparse", "pedigree", "c3"])
def test_tree_order_fit_is_within_1e6_of_reference_order(oracle, abn, golden, name):
    ped, p0, S, B, max_starts, max_rows, max_frac = _cases(golden)[name]
    tree = abn.reduction_tree(ped[:, :3], abn.default_options(strict_order=-1))   # the pedigree's tree (host arithmetic)
    assert tree == CANON
    # the DEFAULT order: the tree, except for pedigrees of up to 16 rows — the bundled one — which are summed serially
    assert abn.reduction_tree(ped[:, :3]) == (1 if ped.shape[0] <= 16 else tree)
    ref = oracle_pipeline(oracle, ped, p0, S, B, 1)
    got = oracle_pipeline(oracle, ped, p0, S, B, tree)
    same, _ = oracle.boot_model(ped, ref["model"], ref["pred"], ref["resid"], p0, p0, 1.0, SEED, 0, 0, B, lanes=tree)
    compare(ref, got, same, name, max_starts, max_rows, max_frac)


def test_strict_order_reports_the_serial_tree_code(abn, golden):
    assert abn.reduction_tree(golden["sparse"][:, :3], abn.default_options(strict_order=1)) == 1


# ------------------------------------------------------------------------------------------------ GPU
def hip_pipeline(abn, ctx, ped, p0, S, B, opts):
    model, pred, resid, extra = ctx.ab_neutral_run(ped, p0, p0, 1.0, S, options=opts)
    raw, info = ctx.boot_model_run(ped, model, pred, resid, p0, p0, 1.0, B, options=opts)
    fits = np.zeros(S, dtype=[("best", "<f8", (4,)), ("status", "<i4"), ("evals", "<i4")])
    fits["best"], fits["status"], fits["evals"] = extra["models"], extra["info"]["status"], extra["info"]["evals"]
    return {"fits": fits, "model": model, "pred": pred, "resid": resid, "raw": raw, "res": info, "info_a": extra["info"]}


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["generated", "sparse", "pedigree", "c3"])
def test_hip_auto_options_against_reference_order(oracle, abn, gpu_ctx, golden, name):
    """the product as shipped (auto options: canonical tree, whatever kernels the launch sizes pick) beside the
    oracle in the REFERENCE's summation order"""
    ped, p0, S, B, max_starts, max_rows, max_frac = _cases(golden)[name]
    ref = oracle_pipeline(oracle, ped, p0, S, B, 1)
    opts = abn.default_options(seed=SEED)
    got = hip_pipeline(abn, gpu_ctx, ped, p0, S, B, opts)
    same, _ = gpu_ctx.boot_model_run(ped, ref["model"], ref["pred"], ref["resid"], p0, p0, 1.0, B, options=opts)
    if name == "generated":
        # the bundled data/ pedigree (C1 / C2, the north star's parity target) is in the reference's
        # order BY DEFAULT — 0 starts and 0 rows apart, every bit
        assert np.all(got["info_a"]["lanes"] == 1) and np.all(got["res"]["lanes"] == 1)
        for k in ("model", "pred", "resid", "raw"):
            assert np.array_equal(got[k], ref[k]), k
        assert np.array_equal(got["info_a"]["evals"], ref["fits"]["evals"]) and np.array_equal(same, ref["raw"])
        max_starts = max_rows = max_frac = 0
    compare(ref, got, same, name, max_starts, max_rows, max_frac)
    if name == "generated":   # the tree on the same pedigree (strict_order = -1) stays inside the bounds of round 3
        max_starts, max_rows, max_frac = _cases(golden)[name][4:]
        topts = abn.default_options(seed=SEED, strict_order=-1)
        tgot = hip_pipeline(abn, gpu_ctx, ped, p0, S, B, topts)
        tsame, _ = gpu_ctx.boot_model_run(ped, ref["model"], ref["pred"], ref["resid"], p0, p0, 1.0, B, options=topts)
        assert np.all(tgot["res"]["lanes"] == CANON)
        compare(ref, tgot, tsame, name + " (tree)", max_starts, max_rows, max_frac)


@pytest.mark.gpu
@pytest.mark.parametrize("name,S,B", [("generated", 1000, 1000), ("sparse", 40, 200), ("pedigree", 40, 200), ("c3", 40, 400)])
def test_hip_strict_order_is_bit_equal_to_reference_order(oracle, abn, gpu_ctx, golden, name, S, B):
    """abn_options.strict_order = 1: serial row-order sums in the fit kernels -> every start, the selection and every
    bootstrap row bit-equal to the oracle's lanes = 1 (C1/C2's pedigree at 1000 starts + 1000 bootstraps)"""
    ped, p0 = _cases(golden)[name][:2]
    ref = oracle_pipeline(oracle, ped, p0, S, B, 1)
    got = hip_pipeline(abn, gpu_ctx, ped, p0, S, B, abn.default_options(seed=SEED, strict_order=1))
    assert np.all(got["info_a"]["lanes"] == 1) and np.all(got["res"]["lanes"] == 1)
    for f in ("status", "iters", "evals"):
        assert np.array_equal(got["info_a"][f], ref["fits"][f]), f
        assert np.array_equal(got["res"][f], ref["res"][f]), f
    ok = ref["fits"]["status"] != 2
    assert np.array_equal(got["fits"]["best"][ok], ref["fits"]["best"][ok])
    assert np.array_equal(got["info_a"]["best_cost"][ok], ref["fits"]["best_cost"][ok])
    for k in ("model", "pred", "resid", "raw"):
        assert np.array_equal(got[k], ref[k]), k


@pytest.mark.gpu
@pytest.mark.parametrize("lanes", [0, 8, 16, 32, 64])
def test_hip_strict_order_fit_batch_every_packing(oracle, abn, gpu_ctx, golden, lanes):
    """the serial sum does not depend on how many lanes a chain has: every packing, resident and streamed rows"""
    rng = np.random.default_rng(77 + lanes)
    for ped, p0, F, iters in ((golden["sparse"], golden["r_p0uu"], 37, 300), (golden["generated"], 0.655, 70, 400),
                             (synthetic_pedigree(rng, 700, 30), 0.8, 9, 60), (synthetic_pedigree(rng, 1500, 12), 0.7, 5, 40)):
        s0 = np.stack([oracle.start_simplex(SEED, 3, s, ped[:, 3].max()) for s in range(F)])
        best, info = gpu_ctx.fit_batch(ped, p0, p0, 1.0, s0, iters,
                                       options=abn.default_options(strict_order=1, lanes_per_chain=lanes))
        want = oracle.fit_batch(ped, p0, p0, 1.0, s0, iters, lanes=1)
        assert np.all(info["lanes"] == 1)
        for f in ("status", "iters", "evals"):
            assert np.array_equal(info[f], want[f]), (lanes, ped.shape, f)
        ok = want["status"] != 2
        assert np.array_equal(best[ok], want["best"][ok])
        assert np.array_equal(info["best_cost"][ok], want["best_cost"][ok])


@pytest.mark.gpu
def test_hip_strict_order_plan_multi_window_and_stream(oracle, abn, gpu_ctx):
    """abn_plan_* under strict order: several windows, and a deep pedigree whose rows are streamed"""
    from alphabeta_rs_amd import synthetic

    gens, D, p0, _ = synthetic.c4_windows(5)
    opts = abn.default_options(seed=SEED, strict_order=1)
    plan = abn.Plan(gpu_ctx, gens, 5, 6, 24, options=opts)
    plan.set_windows(D, p0)
    plan.run()
    out = plan.download()
    plan.close()
    for w in range(5):
        ped = np.concatenate([gens, D[w][:, None]], axis=1)
        ref = oracle_pipeline(oracle, ped, float(p0[w]), 6, 24, 1, window=w)
        assert np.array_equal(out["models"][w], ref["model"]) and np.array_equal(out["raw"][w], ref["raw"])
        assert np.array_equal(out["info_b"]["evals"][w], ref["res"]["evals"])
    deep, dp0 = synthetic.c5_pedigree(every=25)            # 820 rows: resident at 64 lanes; every=12 -> streamed
    streamed = synthetic.c5_pedigree(every=12)[0]          # (both stream variants: materialised observations, index rows)
    for ped, sm in ((deep, 0), (streamed, 0), (streamed, 1)):
        o = abn.default_options(seed=SEED, strict_order=1, max_iters_start=40, max_iters_boot=30, stream_mode=sm)
        plan = abn.Plan(gpu_ctx, ped[:, :3], 1, 3, 5, options=o)
        plan.set_windows(ped[:, 3][None, :], np.array([dp0]))
        plan.run()
        out = plan.download()
        plan.close()
        s0 = np.stack([oracle.start_simplex(SEED, 0, s, ped[:, 3].max()) for s in range(3)])
        fits = oracle.fit_batch(ped, dp0, dp0, 1.0, s0, 40, lanes=1)
        k, model, pred, resid, _ = oracle.select_best(ped, dp0, fits["best"])
        raw, res = oracle.boot_model(ped, model, pred, resid, dp0, dp0, 1.0, SEED, 0, 0, 5, max_iters=30, lanes=1)
        assert np.array_equal(out["models"][0], model) and np.array_equal(out["raw"][0], raw)
        assert np.all(out["info_b"]["lanes"] == 1)
