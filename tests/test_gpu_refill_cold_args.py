"""The persistent fit kernel reads what its cold parts need from the kernel-argument segment, where they need it
(csrc/abn_fit_refill.hpp: ColdArgs), not from registers filled at entry.  Each case below is a persistent, time-sliced
launch at the smallest size the route admits (16 lanes per chain: more than 8192 chains) that exercises arguments only
the cold parts read: the index row and the `raw` table (bound and the plan's own), the window ids, a bootstrap offset,
`skipped`, the start simplices (phase A, no `raw`), and the guard words of an early phase B that is stopped.

Pedigrees of 40 rows (refill<16, 4>) and 105 rows (refill<16, 8>, the C3 topology); 300 iterations at the most, so that
chains outlive a quantum of 256 evaluations and park.  Every case asserts that the launch was the persistent kernel with
a quantum and a tail cap (the restatement below over tests/_route_model.py, and Plan.last_kernels), outputs bit-equal
to the oracle, every chain finished and the error word zero (Plan.sync checks the launch's status words and raises
otherwise; the fit counter), and a tail hand-over within 1..cap (the count depends on the schedule)."""
import ctypes as C

import numpy as np
import pytest

from alphabeta_rs_amd import synthetic

import _parity
import _route_model as RM

pytestmark = pytest.mark.gpu
SEED = 20260101
ITERS = 300
QUANTUM = 256                      # abn_route.hpp: kQuantum
CHAINS = 8200                      # > 2048 wavefronts of four chains


def sliced_route(dev, ped, chains):
    """(lanes, rows per lane, quantum, tail cap) of a whole-plan launch of `chains` chains with auto options, by
    route_launch's arithmetic restated; asserts that it is a persistent one"""
    n = ped.shape[0]
    tmax, k, cs = RM.topology(ped[:, :3])
    lanes = RM.pick_lanes(n, 0, cs)
    ng = RM.WAVE // lanes
    assert not RM.strict_of(n, {}) and not RM.streams(n, k, cs, lanes)
    blocks = -(-chains // ng)
    small, full = dev["persistent_wavefronts_small"], dev["persistent_wavefronts"]
    assert ng > 1 and blocks > small                                   # persistent_by_size
    grid = full if blocks > full else small
    q = (5 * QUANTUM * chains // (grid * ng) // 8 + 63) & ~63
    quantum = min(4 * QUANTUM, max(QUANTUM, q))
    per_cu = (8 if grid == full else 4) if RM.pick_rmax(n, RM.WAVE) <= 2 else 2
    cap = per_cu * dev["compute_units"] if RM.spec_fits(n, tmax, k, 0) else 0
    return lanes, RM.pick_rmax(n, lanes), quantum, cap


def assert_sliced(gpu_ctx, ped, chains, rows, kind, handed):
    lanes, r, quantum, cap = sliced_route(gpu_ctx.device_info(), ped, chains)
    assert (lanes, r) == (16, rows) and quantum > 0 and cap > 0, (lanes, r, quantum, cap)
    assert kind == ("persistent", 16), kind
    assert 1 <= handed <= cap, (handed, cap)


def ped40():
    return RM.boundary_pedigree(40, 12, 30, seed=1), synthetic.TRUE_P0UU


def options(abn, **kw):
    return abn.default_options(seed=SEED, max_iters_boot=ITERS, **kw)


@pytest.fixture(scope="module")
def c3_starts(abn, oracle):
    """the C3 window's ten starts and the selection over them, once"""
    ped, p0 = synthetic.c3_pedigree()
    tree = abn.reduction_tree(ped[:, :3], options(abn))
    s0 = abn.gen_start_simplices(SEED, 0, 10, float(ped[:, 3].max()))
    return ped, p0, tree, oracle.fit_batch(ped, p0, p0, 1.0, s0, 10000, lanes=tree, threads=4)


@pytest.fixture(scope="module")
def c3_many_starts(abn, oracle):
    """8200 starts on the C3 window at 300 iterations, once: several hundred of them reach argmin's fixed point"""
    ped, p0 = synthetic.c3_pedigree()
    tree = abn.reduction_tree(ped[:, :3], options(abn))
    s0 = abn.gen_start_simplices(SEED, 0, CHAINS, float(ped[:, 3].max()))
    return ped, p0, tree, oracle.fit_batch(ped, p0, p0, 1.0, s0, ITERS, lanes=tree, threads=8)


@pytest.fixture(scope="module")
def hip():
    h = C.CDLL("libamdhip64.so")        # the HIP runtime the product library already holds
    h.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    h.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    h.hipFree.argtypes = [C.c_void_p]
    return h


@pytest.mark.parametrize("bound", (True, False), ids=("raw_bound", "own_raw"))
def test_bootstraps_through_the_index_row(abn, gpu_ctx, oracle, hip, c3_starts, bound):
    """the default route (dmode 1, smode 1; one window: the early, guarded phase B): the whole table against the oracle,
    written to a caller's table and to the plan's own"""
    ped, p0, tree, fits = c3_starts
    plan = abn.Plan(gpu_ctx, ped[:, :3], 1, 10, CHAINS, options=options(abn))
    buf = C.c_void_p()
    try:
        if bound:
            assert hip.hipMalloc(C.byref(buf), CHAINS * 7 * 8) == 0
            plan.bind_raw(buf.value)
        plan.set_windows(ped[:, 3][None, :], np.array([p0]))
        plan.run()
        plan.sync()
        out, kinds, handed, cnt = plan.download(), plan.last_kernels(), plan.tail_handed(), plan.counters()
        if bound:
            mine = np.zeros((1, CHAINS, 7))
            assert hip.hipMemcpy(mine.ctypes.data, buf, mine.nbytes, 2) == 0
            _parity.assert_same_bits(mine, out["raw"], "the bound table")
    finally:
        plan.close()
        if buf.value:
            hip.hipFree(buf)
    assert_sliced(gpu_ctx, ped, CHAINS, 8, kinds["boot"], handed[1])
    assert cnt["fits"] == 10 + CHAINS, cnt
    _parity.assert_fits_equal(None, out["info_a"][0], fits)
    _parity.check_selection_and_boot(oracle, ped, p0, out, fits["best"], SEED, ITERS, tree)


def test_seven_windows_with_window_ids(abn, gpu_ctx, oracle):
    """the nullable window-id array: 7 x 1172 chains on 40 rows, every window under its own Philox window id"""
    ped, p0 = ped40()
    ids = [5, 0, 11, 3, 22, 4, 9]
    W, S, B = len(ids), 6, 1172
    D = np.abs(ped[:, 3][None, :] * np.random.default_rng(3).uniform(0.8, 1.25, (W, 1)))
    o = options(abn)
    out, kinds, handed = _parity.run_plan(abn, gpu_ctx, ped, p0, S, B, o, ids=ids, D=D)
    assert_sliced(gpu_ctx, ped, W * B, 4, kinds["boot"], handed[1])
    tree = abn.reduction_tree(ped[:, :3], o)
    for w in (0, 4, W - 1):
        pw = np.concatenate([ped[:, :3], D[w][:, None]], axis=1)
        s0 = abn.gen_start_simplices(SEED, ids[w], S, float(D[w].max()))
        fits = oracle.fit_batch(pw, p0, p0, 1.0, s0, 10000, lanes=tree, threads=4)
        _parity.assert_fits_equal(None, out["info_a"][w], fits, w)
        _parity.check_selection_and_boot(oracle, pw, p0, out, fits["best"], SEED, ITERS, tree, label=w, window=w, ids=ids)


def test_bootstrap_offset(abn, gpu_ctx, oracle):
    """Philox counters with a nonzero bootstrap offset: bootstrap b of the plan draws the streams of 1000 + b"""
    ped, p0 = ped40()
    o = options(abn)
    out, kinds, handed = _parity.run_plan(abn, gpu_ctx, ped, p0, 6, CHAINS, o, boot_offset=1000)
    assert_sliced(gpu_ctx, ped, CHAINS, 4, kinds["boot"], handed[1])
    tree = abn.reduction_tree(ped[:, :3], o)
    fits = oracle.fit_batch(ped, p0, p0, 1.0, abn.gen_start_simplices(SEED, 0, 6, float(ped[:, 3].max())), 10000, lanes=tree,
                            threads=4)
    _parity.check_selection_and_boot(oracle, ped, p0, out, fits["best"], SEED, ITERS, tree, boot_offset=1000)


def run_starts(abn, gpu_ctx, ped, p0, **opts):
    """8200 starts (phase A on start simplices: smode 0, dmode 0, no `raw`) and four bootstraps"""
    plan = abn.Plan(gpu_ctx, ped[:, :3], 1, CHAINS, 4, options=options(abn, max_iters_start=ITERS, **opts))
    plan.set_windows(ped[:, 3][None, :], np.array([p0]))
    plan.run()
    plan.sync()
    res = plan.download(), plan.last_kernels(), plan.tail_handed(), plan.counters()
    plan.close()
    return res


def assert_starts(oracle, ped, p0, out, fits):
    _parity.assert_fits_equal(None, out["info_a"][0], fits)
    best, model, pred, resid, _ = oracle.select_best(ped, p0, fits["best"])
    assert out["best_start"][0] == best and np.array_equal(out["models"][0], model)
    assert np.array_equal(out["pred"][0], pred) and np.array_equal(out["resid"][0], resid)


@pytest.mark.parametrize("no_skip", (0, 1))
def test_stuck_fits_with_and_without_the_skip(abn, gpu_ctx, oracle, c3_many_starts, no_skip):
    """`skipped` is written (0) / the repeated iterations are executed (1): the same table either way, the oracle's"""
    ped, p0, _, fits = c3_many_starts
    at_max = (fits["status"] == 1) & (fits["iters"] == ITERS)
    assert at_max.sum() > 300, at_max.sum()
    out, kinds, handed, cnt = run_starts(abn, gpu_ctx, ped, p0, no_fixed_point_skip=no_skip)
    assert_sliced(gpu_ctx, ped, CHAINS, 8, kinds["starts"], handed[0])
    assert cnt["fits"] == CHAINS + 4, cnt
    print("evaluations skipped in phase A:", cnt["evals_skipped_starts"])
    if no_skip:
        assert cnt["evals_skipped_starts"] == 0, cnt
    else:     # some of the chains that end at the iteration limit are at the fixed point; each skips an even count
        assert 0 < cnt["evals_skipped_starts"] <= 2 * ITERS * int(at_max.sum()) and cnt["evals_skipped_starts"] % 2 == 0, cnt
    assert cnt["evals"] == int(fits["evals"].sum()) + int(out["info_b"]["evals"].sum()), cnt   # skipped ones counted as run
    assert_starts(oracle, ped, p0, out, fits)


def test_phase_a_on_start_simplices(abn, gpu_ctx, oracle):
    """the start-simplex route on 40 rows: refill<16, 4> reads simplex0 and D, and has no `raw` to write"""
    ped, p0 = ped40()
    out, kinds, handed, cnt = run_starts(abn, gpu_ctx, ped, p0)
    assert_sliced(gpu_ctx, ped, CHAINS, 4, kinds["starts"], handed[0])
    assert cnt["fits"] == CHAINS + 4, cnt
    tree = abn.reduction_tree(ped[:, :3], options(abn))
    s0 = abn.gen_start_simplices(SEED, 0, CHAINS, float(ped[:, 3].max()))
    fits = oracle.fit_batch(ped, p0, p0, 1.0, s0, ITERS, lanes=tree, threads=8)
    assert_starts(oracle, ped, p0, out, fits)
    _parity.check_selection_and_boot(oracle, ped, p0, out, fits["best"], SEED, ITERS, tree)


def test_guarded_early_phase_b_that_is_stopped(abn, gpu_ctx, oracle):
    """window 4 of the C4 set: the best start is the longest chain, so the early phase B is stopped through its guard
    word and redone (tests/test_gpu_early_bootstraps.py builds the same miss at 1000 iterations)"""
    gens, D, p0s, _ = synthetic.c4_windows(1, window_offset=4)
    ped, p0 = np.concatenate([gens, D[0][:, None]], axis=1), float(p0s[0])
    o = options(abn)
    tree = abn.reduction_tree(gens, o)
    fits = oracle.fit_batch(ped, p0, p0, 1.0, abn.gen_start_simplices(SEED, 4, 10, float(ped[:, 3].max())), 10000, lanes=tree,
                            threads=4)
    best = int(oracle.select_best(ped, p0, fits["best"])[0])
    length = np.where((fits["status"] == 1) & (fits["iters"] == 10000), 0, fits["iters"])
    assert best == np.argsort(length, kind="stable")[-1], (best, length)            # a miss by construction
    plan = abn.Plan(gpu_ctx, gens, 1, 10, CHAINS, window_offset=4, options=o)
    plan.set_early_bootstraps(1)
    plan.set_windows(D, p0s)
    plan.run()
    plan.sync()
    out, st, kinds, handed, cnt = plan.download(), plan.early_bootstraps(), plan.last_kernels(), plan.tail_handed(), plan.counters()
    plan.close()
    assert st["eligible"] and st["miss"] and st["parked"] >= 1, st
    assert_sliced(gpu_ctx, ped, CHAINS, 8, kinds["boot"], handed[1])
    assert cnt["fits"] == 10 + CHAINS, cnt                                          # one phase A, one phase B
    _parity.assert_fits_equal(None, out["info_a"][0], fits)
    _parity.check_selection_and_boot(oracle, ped, p0, out, fits["best"], SEED, ITERS, tree, ids=[4])
