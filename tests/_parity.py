"""What the GPU parity tests share: a random valid pedigree, one plan run, and the bit-exact comparisons with the oracle
(fits; the selection and the bootstrap rows replayed from it)."""
import numpy as np

WAVE = 64


def synthetic_pedigree(rng, n, tmax, frac_t0=0.3):
    """random valid (t0,t1,t2,D) rows: t0 <= t1,t2 <= tmax"""
    t0 = np.where(rng.random(n) < frac_t0, rng.integers(0, max(1, tmax // 2), n), 0)
    t1 = t0 + rng.integers(0, tmax - t0 + 1)
    t2 = t0 + rng.integers(0, tmax - t0 + 1)
    d = np.abs(rng.normal(0.01, 0.004, n))
    return np.stack([t0, t1, t2, d], axis=1).astype(np.float64)


def sample_chains(n, lanes, seed=20261016, extra=5):
    """chain indices: first, last, the first chain of the last (partly filled) wavefront, and `extra` seeded others"""
    ng = WAVE // lanes
    pick = {0, n - 1, ((n - 1) // ng) * ng}
    pick |= set(np.random.default_rng(seed).choice(n, min(extra, n), replace=False).tolist())
    return np.array(sorted(pick))


def assert_same_bits(got, want, what):
    """bit for bit: uint64 views, two NaN count as equal (payloads are not part of the contract)"""
    got, want = np.ascontiguousarray(got, dtype=np.float64).reshape(-1), np.ascontiguousarray(want, dtype=np.float64).reshape(-1)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    same = (got.view(np.uint64) == want.view(np.uint64)) | (np.isnan(got) & np.isnan(want))
    assert same.all(), f"{what}: entries {np.flatnonzero(~same)[:8]} differ: {got[~same][:4]} != {want[~same][:4]}"


def assert_fits_equal(best, info, want, label=None):
    """status, iterations, evaluations, and — on every fit that found a finite best — the cost and the vertex
    (`best` None: the vertices were not downloaded)"""
    for f in ("status", "iters", "evals"):
        assert np.array_equal(info[f], want[f]), (label, f)
    ok = want["status"] != 2
    if best is not None:
        assert np.array_equal(best[ok], want["best"][ok]), label
    assert np.array_equal(info["best_cost"][ok], want["best_cost"][ok]), label


def run_plan(abn, ctx, ped, p0, S, B, o, boot_offset=0, ids=None, D=None, sweep=None):
    """S starts and B bootstraps per window: (download(), last_kernels(), tail_handed()).  One window with the pedigree's
    own observations, or — `ids` given — one window per explicit Philox window id (Plan.set_window_ids), with the rows of
    `D` (default: the pedigree's observations for each) and `p0` for all; `sweep`: Plan.set_stream_sweep"""
    W = 1 if ids is None else len(ids)
    D = np.tile(ped[:, 3], (W, 1)) if D is None else np.asarray(D, dtype=np.float64).reshape(W, ped.shape[0])
    plan = abn.Plan(ctx, ped[:, :3], W, S, B, boot_offset=boot_offset, options=o)
    if ids is not None:
        plan.set_window_ids(np.asarray(ids, dtype=np.uint32))
    if sweep is not None:
        plan.set_stream_sweep(sweep)
    plan.set_windows(D, np.full(W, p0))
    plan.run()
    out = plan.download()
    kinds, handed = plan.last_kernels(), plan.tail_handed()
    plan.close()
    return out, kinds, handed


def check_selection_and_boot(oracle, ped, p0, out, best_a, seed, iters_b, tree, label=None, rows=None,
                             info_fields=("iters", "evals", "status"), window=0, ids=None, boot_offset=0):
    """best_start / model / pred / resid from the oracle's selection over `best_a`, then the bootstrap rows (all, or the
    sampled `rows`) replayed one by one: the raw rows and `info_fields` of info_b.  `window`: the plan's window compared
    (`ped` carries that window's observations); its Philox window id is ids[window], or `window` itself without `ids`;
    `boot_offset`: the plan's (bootstrap b draws from the streams of boot_offset + b)"""
    w = window
    wid = int(w if ids is None else ids[w])
    kk, model, pred, resid, _ = oracle.select_best(ped, p0, best_a)
    assert out["best_start"][w] == kk and np.array_equal(out["models"][w], model), label
    assert np.array_equal(out["pred"][w], pred) and np.array_equal(out["resid"][w], resid), label
    B = out["raw"].shape[1]
    for b0, nb in ([(0, B)] if rows is None else [(int(b), 1) for b in rows]):
        raw, res = oracle.boot_model(ped, model, pred, resid, p0, p0, 1.0, seed, wid, boot_offset + b0, nb, max_iters=iters_b,
                                     lanes=tree, threads=4)
        assert np.array_equal(out["raw"][w, b0:b0 + nb], raw, equal_nan=True), (label, b0)
        for f in info_fields:
            assert np.array_equal(out["info_b"][f][w, b0:b0 + nb], res[f]), (label, b0, f)
