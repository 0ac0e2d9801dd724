"""What the GPU parity tests share: a random valid pedigree, one plan run, and the bit-exact comparisons with the oracle
(fits; the selection and the bootstrap rows replayed from it)."""
import numpy as np


def synthetic_pedigree(rng, n, tmax, frac_t0=0.3):
    """random valid (t0,t1,t2,D) rows: t0 <= t1,t2 <= tmax"""
    t0 = np.where(rng.random(n) < frac_t0, rng.integers(0, max(1, tmax // 2), n), 0)
    t1 = t0 + rng.integers(0, tmax - t0 + 1)
    t2 = t0 + rng.integers(0, tmax - t0 + 1)
    d = np.abs(rng.normal(0.01, 0.004, n))
    return np.stack([t0, t1, t2, d], axis=1).astype(np.float64)


def assert_fits_equal(best, info, want, label=None):
    """status, iterations, evaluations, and — on every fit that found a finite best — the cost and the vertex
    (`best` None: the vertices were not downloaded)"""
    for f in ("status", "iters", "evals"):
        assert np.array_equal(info[f], want[f]), (label, f)
    ok = want["status"] != 2
    if best is not None:
        assert np.array_equal(best[ok], want["best"][ok]), label
    assert np.array_equal(info["best_cost"][ok], want["best_cost"][ok]), label


def run_plan(abn, ctx, ped, p0, S, B, o, boot_offset=0):
    """one window, S starts and B bootstraps: (download(), last_kernels(), tail_handed())"""
    plan = abn.Plan(ctx, ped[:, :3], 1, S, B, boot_offset=boot_offset, options=o)
    plan.set_windows(ped[:, 3][None, :], np.array([p0]))
    plan.run()
    out = plan.download()
    kinds, handed = plan.last_kernels(), plan.tail_handed()
    plan.close()
    return out, kinds, handed


def check_selection_and_boot(oracle, ped, p0, out, best_a, seed, iters_b, tree, label=None, rows=None,
                             info_fields=("iters", "evals", "status")):
    """best_start / model / pred / resid from the oracle's selection over `best_a`, then the bootstrap rows (all, or the
    sampled `rows`) replayed one by one: the raw rows and `info_fields` of info_b"""
    kk, model, pred, resid, _ = oracle.select_best(ped, p0, best_a)
    assert out["best_start"][0] == kk and np.array_equal(out["models"][0], model), label
    assert np.array_equal(out["pred"][0], pred) and np.array_equal(out["resid"][0], resid), label
    B = out["raw"].shape[1]
    for b0, nb in ([(0, B)] if rows is None else [(int(b), 1) for b in rows]):
        raw, res = oracle.boot_model(ped, model, pred, resid, p0, p0, 1.0, seed, 0, b0, nb, max_iters=iters_b, lanes=tree,
                                     threads=4)
        assert np.array_equal(out["raw"][0, b0:b0 + nb], raw, equal_nan=True), (label, b0)
        for f in info_fields:
            assert np.array_equal(out["info_b"][f][0, b0:b0 + nb], res[f]), (label, b0, f)
