"""One preparation launch per step (abn_step_prepare_kernel; alphabeta_rs_amd/csrc/abn_prepare.hpp): the plan words, the
FIFO of phase B's slot and the redo's own FIFO are cleared at the head of the step and nowhere else.  What that must not
change is any byte of any output, whatever the step before left behind: a stopped early phase B leaves its FIFO dirty, a
redo that ran leaves the redo's.

All on the C3 topology (105 rows), S = 10, B = 8200 (the smallest plan the route gives to the persistent kernel, hence the
smallest eligible one), seed 20260101.  Which observations hit and which miss is derived from the oracle (best start and the
starts' finishing order in iterations, as tests/test_gpu_early_bootstraps.py does) and asserted against what the plan
reports, so that no case can pass vacuously."""
import numpy as np
import pytest

from alphabeta_rs_amd import synthetic

SEED, S, B, QUORUM = 20260101, 10, 8200, 8
ITERS_A = 10000
WOFF = 4                          # the fixed window offset of case 1: window 4 misses at its own offset
CANDIDATES = (11, 2, 4, 5, 7, 9)  # observations of these windows of synthetic.c4_windows are searched with the oracle
KEYS = ("models", "pred", "resid", "raw", "best_start", "info_a", "info_b")
pytestmark = pytest.mark.gpu


def assert_same_bytes(a, b, label=None):
    for k in KEYS:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), (label, k)


def classify(abn, oracle, ped, p0, woff):
    """'hit' / 'miss' / None (too close to call) of one window's observations under window offset woff, from the oracle:
    a hit when the best start is among the first QUORUM finishers and the ninth is well behind the eighth (the parked set
    is then the same every time), a miss when the best start finishes behind the eighth by a margin"""
    tree = abn.reduction_tree(ped[:, :3], abn.default_options(seed=SEED))
    s0 = abn.gen_start_simplices(SEED, woff, S, float(ped[:, 3].max()))
    fits = oracle.fit_batch(ped, p0, p0, 1.0, s0, ITERS_A, lanes=tree)
    best = int(oracle.select_best(ped, p0, fits["best"])[0])
    length = np.where((fits["status"] == 1) & (fits["iters"] == ITERS_A), 0, fits["iters"])   # stuck: ends at once
    order = [int(i) for i in np.argsort(length, kind="stable")]
    eighth, ninth = length[order[QUORUM - 1]], length[order[QUORUM]]
    if best in order[:QUORUM] and ninth > 1.15 * eighth:
        return "hit"
    if best in order[QUORUM:] and length[best] > 1.05 * eighth:
        return "miss"
    return None


def observations(window):
    gens, D, p0, _ = synthetic.c4_windows(1, window_offset=window)
    return np.concatenate([gens, D[0][:, None]], axis=1), float(p0[0])


def fresh(abn, ctx, ped, p0, woff, mode, n_windows=1, n_boot=B, d=None, p=None):
    """download, early_bootstraps, counters, tail_handed of one run() of a new plan"""
    plan = abn.Plan(ctx, ped[:, :3], n_windows, S, n_boot, window_offset=woff, options=abn.default_options(seed=SEED))
    plan.set_early_bootstraps(mode)
    plan.set_windows(ped[:, 3][None, :] if d is None else d, np.array([p0]) if p is None else p)
    plan.run()
    res = plan.download(), plan.early_bootstraps(), plan.counters(), plan.tail_handed()
    plan.close()
    return res


@pytest.fixture(scope="module")
def sequence(abn, oracle, gpu_ctx):
    """Computed once and never changed: four windows' observations in the order miss, hit, miss, hit under offset WOFF (the
    oracle's call), and for each a fresh plan's run with early bootstraps on and off"""
    kinds = {}
    for w in CANDIDATES:
        ped, p0 = observations(w)
        kinds[w] = classify(abn, oracle, ped, p0, WOFF)
    misses = [w for w in CANDIDATES if kinds[w] == "miss"]
    hits = [w for w in CANDIDATES if kinds[w] == "hit"]
    assert len(misses) >= 2 and len(hits) >= 2 and 4 in misses, kinds
    seq = [misses[0], hits[0], misses[1], hits[1]]
    out = []
    for w in seq:
        ped, p0 = observations(w)
        on = fresh(abn, gpu_ctx, ped, p0, WOFF, 1)
        off = fresh(abn, gpu_ctx, ped, p0, WOFF, 0)
        out.append(dict(window=w, kind=kinds[w], ped=ped, p0=p0, on=on, off=off))
    return out


def test_one_plan_through_miss_hit_miss_hit(abn, gpu_ctx, sequence):
    """Case 1: every step starts on what the last one left — a stopped phase B's FIFO and a used redo FIFO after a miss, a
    raised miss word, parked rows — and computes the bytes of a fresh plan, and of the plan with early bootstraps off"""
    assert [s["kind"] for s in sequence] == ["miss", "hit", "miss", "hit"]
    plan = abn.Plan(gpu_ctx, sequence[0]["ped"][:, :3], 1, S, B, window_offset=WOFF, options=abn.default_options(seed=SEED))
    for step, s in enumerate(sequence):
        plan.set_windows(s["ped"][:, 3][None, :], np.array([s["p0"]]))
        plan.run()
        out, st, cnt = plan.download(), plan.early_bootstraps(), plan.counters()
        label = (step, s["window"], s["kind"])
        f_out, f_st, f_cnt, _ = s["on"]
        assert st["eligible"] and st["quorum"] == QUORUM and st["miss"] == (s["kind"] == "miss"), (label, st)
        assert f_st["miss"] == st["miss"], (label, st, f_st)                      # the oracle's call is the device's
        if s["kind"] == "hit":      # both stragglers are far behind the eighth finisher: both park, every time
            assert st == f_st and st["parked"] == S - QUORUM, (label, st, f_st)
        else:                       # the ninth may finish in the iterations it takes the flag to be seen (window 4: 7 left)
            assert 1 <= st["parked"] <= S - QUORUM and 1 <= f_st["parked"] <= S - QUORUM, (label, st, f_st)
        assert not s["off"][1]["miss"] and s["off"][1]["parked"] == 0, (label, s["off"][1])
        assert_same_bytes(out, f_out, label)
        assert_same_bytes(out, s["off"][0], label)
        assert cnt == f_cnt == s["off"][2], (label, cnt, f_cnt, s["off"][2])
    plan.close()


def test_mixed_entry_points_on_one_plan(abn, gpu_ctx, sequence):
    """Case 2: run(), run_phase(0), run_phase(1), run() on one plan (a hit).  The preparation serves both entry points:
    each download is a fresh plan's, and so are counters(), tail_handed() and early_bootstraps() — after run() and after
    run_phase(0), which leaves the early run's phase B in place, those of a fresh plan's run(); after run_phase(1), which
    replaces it with a late launch, those of a fresh plan taken through run_phase(0), run_phase(1).

    tail_handed() of phase B is a count of the schedule, not of the inputs: how many chains are still running when the
    queue runs dry.  Two fresh plans on the same inputs gave 624 and 633 on one MI355X, so it is held to what a fresh plan's
    fixes — nothing handed in phase A, something in phase B, within the tail's capacity of 1024 — and both figures are
    printed.  That no status word carries over from the step before is held exactly all the same: every synchronisation
    compares the slot's count of finished fits with the launch's chains (verify_persistent) and raises on any other."""
    s = sequence[1]
    assert s["kind"] == "hit"
    f_out, f_st, f_cnt, f_handed = s["on"]

    def armed():
        plan = abn.Plan(gpu_ctx, s["ped"][:, :3], 1, S, B, window_offset=WOFF, options=abn.default_options(seed=SEED))
        plan.set_windows(s["ped"][:, 3][None, :], np.array([s["p0"]]))
        return plan

    phases = armed()
    phases.run_phase(0)
    phases.run_phase(1)
    p_out, p_st, p_cnt, p_handed = phases.download(), phases.early_bootstraps(), phases.counters(), phases.tail_handed()
    phases.close()
    assert_same_bytes(p_out, f_out, "phases")
    assert p_st == {"eligible": True, "quorum": QUORUM, "parked": 0, "miss": False} and p_cnt == f_cnt, (p_st, p_cnt, f_cnt)

    plan = armed()
    last_ms = None
    for step, (entry, want_st, want_handed) in enumerate((("run", f_st, f_handed), ("a", f_st, f_handed),
                                                          ("b", p_st, p_handed), ("run", f_st, f_handed))):
        if entry == "run":
            plan.run()
        else:
            plan.run_phase(0 if entry == "a" else 1)
        out, st, cnt, handed = plan.download(), plan.early_bootstraps(), plan.counters(), plan.tail_handed()
        print("step", step, entry, "early", st, "handed", handed, "fresh", want_handed)
        assert_same_bytes(out, f_out, (step, entry))
        assert st == want_st and cnt == f_cnt, (step, entry, st, want_st, cnt, f_cnt)
        assert handed[0] == want_handed[0] == 0 and 0 < handed[1] <= 1024 and 0 < want_handed[1] <= 1024, (step, entry, handed, want_handed)
        # the three timed spans, from four records per step: each is that of the launches it names, and a phase run on its
        # own leaves the other phase's spans exactly as they were (the same records)
        ms = plan.kernel_ms()
        print("step", step, entry, "kernel_ms", ms)
        assert 0.1 < ms["fit_starts"] < 5.0 and 0.0 < ms["select"] < 0.2 and 0.5 < ms["fit_boot"] < 20.0, (step, entry, ms)
        if entry == "a":
            assert ms["fit_boot"] == last_ms["fit_boot"], (step, ms, last_ms)
        if entry == "b":
            assert ms["fit_starts"] == last_ms["fit_starts"] and ms["select"] == last_ms["select"], (step, ms, last_ms)
        last_ms = ms
    plan.close()


@pytest.mark.parametrize("case", ("plain_resident", "two_windows"))
def test_plans_without_early_bootstraps_compute_the_same(abn, gpu_ctx, case):
    """Case 3: an ineligible plan (B = 8192: the plain resident kernel) and a two-window plan — the default against early
    bootstraps switched off, twice in a row on one plan and through the phases"""
    W, nb = (1, 8192) if case == "plain_resident" else (2, B)
    gens, D, p0, _ = synthetic.c4_windows(W, window_offset=WOFF)

    def plan_with(mode):
        plan = abn.Plan(gpu_ctx, gens, W, S, nb, window_offset=WOFF, options=abn.default_options(seed=SEED))
        plan.set_early_bootstraps(mode)
        plan.set_windows(D, p0)
        return plan

    ref = plan_with(0)
    ref.run()
    want, want_cnt, want_kinds = ref.download(), ref.counters(), ref.last_kernels()
    assert ref.early_bootstraps() == {"eligible": False, "quorum": 0, "parked": 0, "miss": False}
    ref.close()
    assert want_kinds["boot"][0] == ("resident" if case == "plain_resident" else "persistent"), want_kinds
    plan = plan_with(1)
    for step, entry in enumerate(("run", "run", "a", "b", "run")):
        if entry == "run":
            plan.run()
        else:
            plan.run_phase(0 if entry == "a" else 1)
        out, cnt, st = plan.download(), plan.counters(), plan.early_bootstraps()
        assert st == {"eligible": False, "quorum": 0, "parked": 0, "miss": False}, (case, step, st)
        assert_same_bytes(out, want, (case, step, entry))
        assert cnt == want_cnt, (case, step, cnt, want_cnt)
    plan.close()
