"""Two grid-stride loops past their first trip: abn_rows_kernel (abn_bootstrap_rows: at most 4096 blocks of 256 threads)
and abn_make_dstar_kernel (the materialised bootstrap observations of a streamed plan: at most 64 blocks of 256 threads per
CU).  A loop that stops after one trip leaves the rows beyond the grid unwritten; everything is compared bit for bit."""
import numpy as np
import pytest

from _parity import assert_fits_equal, assert_same_bits, check_selection_and_boot, sample_chains, synthetic_pedigree

pytestmark = pytest.mark.gpu

ROWS_GRID = 4096 * 256      # abn_bootstrap_rows' largest grid, in threads


def _model_block():
    """4096 distinct (alpha, beta, weight, intercept): plausible fits, and rows whose derived columns are special —
    alpha + beta == 0 (0 / 0: NaN), a negative alpha, infinities, subnormals"""
    rng = np.random.default_rng(31)
    n = ROWS_GRID // 256
    m = np.stack([10.0 ** rng.uniform(-6, -2, n), 10.0 ** rng.uniform(-6, -2, n), rng.uniform(0, 1, n),
                  rng.normal(0.0, 0.01, n)], axis=1)
    m[5::16, 0] = -m[5::16, 0]                      # a negative alpha
    m[7::64, 0] = -m[7::64, 1]                      # alpha + beta == 0
    m[9::128, :2] = 0.0                             # ... both zero
    m[11::128, 0] = np.inf
    m[13::128, 1] = -np.inf
    m[15::64, 0] = 5e-324 * rng.integers(1, 1 << 20, m[15::64, 0].shape)     # subnormal alpha
    m[17::128, :2] = (1e-310, 2e-310)
    m[:, 3] += np.arange(n) * 1e-9                  # distinct rows whatever the above did
    assert len({r.tobytes() for r in m}) == n
    return m


def test_bootstrap_rows_past_one_grid(gpu_ctx, oracle):
    block = _model_block()
    nb = block.shape[0]
    total = ROWS_GRID + 300                          # the last 300 rows belong to the second trip of the first 300 threads
    models = np.tile(block, (total // nb + 1, 1))[:total]
    raw = gpu_ctx.bootstrap_rows(models)
    assert raw.shape == (total, 7)
    want = np.stack([oracle.bootstrap_row(m) for m in block])
    assert np.isnan(want).any() and np.isinf(want).any() and (want[:, 0] < 0).any()
    assert_same_bits(raw[:nb], want, "the first block")
    assert raw.tobytes() == np.tile(raw[:nb], (total // nb + 1, 1))[:total].tobytes()
    assert_same_bits(raw[ROWS_GRID:], want[:300], "the rows past the grid")


def test_materialised_observations_past_one_grid(abn, gpu_ctx, oracle):
    """N = 1100 (streamed at every lane count), two windows, and enough bootstraps for W B N observations to pass
    abn_make_dstar_kernel's grid: the plan with materialised observations (stream_mode 0) against the same plan gathering
    through the index rows (stream_mode 1: no such kernel) byte for byte, and a sample of both windows against the oracle"""
    cus = gpu_ctx.device_info()["compute_units"]
    N, W, S, ia, ib, seed = 1100, 2, 2, 20, 15, 41
    B = (64 * cus * 256 * 105 // 100) // (W * N) + 1
    assert W * B * N > 64 * cus * 256 * 1.05
    rng = np.random.default_rng(77)
    true = np.array([1e-4, 5e-4, 0.03, 1e-3])
    ped = synthetic_pedigree(rng, N, 12)
    dt, _ = oracle.divergence(ped, 0.25, 0.75, *true[:3], table=True)
    ped[:, 3] = np.maximum(true[3] + dt + rng.normal(0, 2e-4, N), 0)
    D = np.stack([ped[:, 3], ped[:, 3] * 1.1])
    p0 = 0.75
    outs = {}
    for mode in (0, 1):
        o = abn.default_options(seed=seed, max_iters_start=ia, max_iters_boot=ib, stream_mode=mode)
        plan = abn.Plan(gpu_ctx, ped[:, :3], W, S, B, options=o)
        plan.set_windows(D, np.full(W, p0))
        plan.run()
        outs[mode] = plan.download()
        kinds = plan.last_kernels()
        plan.close()
        assert kinds["boot"] == ("stream", 64), kinds
    out = outs[0]
    for k in ("models", "pred", "resid", "raw", "info_a", "info_b", "best_start"):
        assert out[k].tobytes() == outs[1][k].tobytes(), k
    tree = abn.reduction_tree(ped[:, :3], o)
    assert tree == 64 | (3 << 8) and np.all(out["info_b"]["lanes"] == tree)
    for w, rows in ((0, sample_chains(B, 64)), (1, np.array([0, B - 1]))):
        pw = np.concatenate([ped[:, :3], D[w][:, None]], axis=1)
        s0 = abn.gen_start_simplices(seed, w, S, D[w].max())
        fits = oracle.fit_batch(pw, p0, p0, 1.0, s0, ia, lanes=tree, table=True, threads=4)
        assert_fits_equal(None, out["info_a"][w], fits, w)
        check_selection_and_boot(oracle, pw, p0, out, fits["best"], seed, ib, tree, w, rows=rows, window=w)
