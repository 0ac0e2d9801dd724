"""A plan's step through every entry point in turn (abn_plan_run, abn_plan_run_phase): one sequence of enqueues drives
them all, and the record of the last run of each phase is kept in one place.  Sequences that nothing else pins:

  * both phases time-sliced on one plan — phase A parks in FIFO region 0 and leaves it dirty, so that phase B's launch
    has to clear it itself (abn_prepare.hpp: prep_launch) — through run(), run(), run_phase(0), run_phase(1), run();
  * window groups through run(), run_phase(0), run_phase(1), run(), with the three timed spans;
  * counters() and kernel_ms() of a plan on a second device while the first is the thread's current one.

Every comparison is of bytes, against the same plan on an independent path (window groups never run persistent and use
no FIFO; one group runs on the context's stream without fork or join), and last_kernels() is asserted after every step so
that no case passes on another route."""
import numpy as np
import pytest

from test_gpu_step_prepare import assert_same_bytes

SEED = 77
pytestmark = pytest.mark.gpu


def windows(ped, W):
    """the observations of tests/test_gpu_parity.py::test_plan_multi_window_matches_per_window_runs, W <= 3 windows"""
    rng = np.random.default_rng(21)
    D = np.abs(ped[:, 3][None, :] * rng.uniform(0.8, 1.2, (3, 1)) + rng.normal(0, 1e-4, (3, ped.shape[0])))
    return D[:W].copy(), np.array([0.99, 0.985, 0.992])[:W]


def step(plan, entry):
    if entry == "run":
        plan.run()
    else:
        plan.run_phase(0 if entry == "a" else 1)
    return plan.download(), plan.counters(), plan.last_kernels(), plan.tail_handed()


def test_both_phases_time_sliced_through_mixed_entry_points(abn, gpu_ctx, golden):
    """W = 2, S = B = 4100 on the sparse pedigree (78 rows) at 16 lanes per chain: 8200 chains per phase, the smallest
    count the route gives to the persistent kernel at four chains per wavefront (more than 8192; the boundary of B = 8200
    in tests/test_gpu_step_prepare.py), so both phases are persistent and time-sliced in region 0 of the one FIFO.  A
    requested tree has no tail hand-over."""
    ped = golden["sparse"]
    W, S, B = 2, 4100, 4100
    D, p0 = windows(ped, W)

    def plan_with(groups):
        o = abn.default_options(seed=SEED, lanes_per_chain=16, strict_order=-1, window_groups=groups)
        plan = abn.Plan(gpu_ctx, ped[:, :3], W, S, B, options=o)
        plan.set_windows(D, p0)
        return plan

    ref = plan_with(2)
    want, want_cnt, ref_kinds, ref_handed = step(ref, "run")
    ref.close()
    assert "persistent" not in (ref_kinds["starts"][0], ref_kinds["boot"][0]) and ref_handed == (0, 0), (ref_kinds, ref_handed)
    assert want_cnt["fits"] == W * (S + B), want_cnt

    plan = plan_with(1)
    for n, entry in enumerate(("run", "run", "a", "b", "run")):
        out, cnt, kinds, handed = step(plan, entry)
        assert kinds == {"starts": ("persistent", 16), "boot": ("persistent", 16)}, (n, entry, kinds)
        assert_same_bytes(out, want, (n, entry))
        assert cnt == want_cnt, (n, entry, cnt, want_cnt)
        assert handed == (0, 0), (n, entry, handed)
    plan.close()


def test_window_groups_through_mixed_entry_points(abn, gpu_ctx, golden):
    """W = 3, S = 4, B = 12 in two window groups: run(), run_phase(0), run_phase(1), run() against one group.  A phase run
    on its own leaves the other phase's spans on the same event records: the same milliseconds, exactly."""
    ped = golden["sparse"]
    W, S, B = 3, 4, 12
    D, p0 = windows(ped, W)

    def plan_with(groups):
        plan = abn.Plan(gpu_ctx, ped[:, :3], W, S, B,
                        options=abn.default_options(seed=SEED, lanes_per_chain=16, window_groups=groups))
        plan.set_windows(D, p0)
        return plan

    ref = plan_with(1)
    want, want_cnt, want_kinds, _ = step(ref, "run")
    ref.close()
    assert want_cnt["fits"] == W * (S + B), want_cnt

    plan = plan_with(2)
    last_ms = None
    for n, entry in enumerate(("run", "a", "b", "run")):
        out, cnt, kinds, handed = step(plan, entry)
        assert kinds == want_kinds and kinds["starts"][1] == kinds["boot"][1] == 16, (n, entry, kinds, want_kinds)
        assert "persistent" not in (kinds["starts"][0], kinds["boot"][0]) and handed == (0, 0), (n, entry, kinds, handed)
        assert_same_bytes(out, want, (n, entry))
        assert cnt == want_cnt, (n, entry, cnt, want_cnt)
        ms = plan.kernel_ms()
        assert ms["fit_starts"] > 0 and ms["select"] > 0 and ms["fit_boot"] > 0, (n, entry, ms)
        if entry == "a":
            assert ms["fit_boot"] == last_ms["fit_boot"], (n, ms, last_ms)
        if entry == "b":
            assert ms["fit_starts"] == last_ms["fit_starts"] and ms["select"] == last_ms["select"], (n, ms, last_ms)
        last_ms = ms
    plan.close()


def test_plan_on_a_second_device_reads_its_own_device(abn, gpu_ctx, golden):
    """counters() and kernel_ms() set the plan's device themselves: taken from a plan on device 1 while device 0 is the
    thread's current device (every call on gpu_ctx's plan makes it so), they are those of the same plan on device 0."""
    if abn.device_count() < 2:
        pytest.skip("one device visible: a plan on a second device needs two")
    ped = golden["sparse"]
    W, S, B = 3, 4, 12
    D, p0 = windows(ped, W)
    o = abn.default_options(seed=SEED, lanes_per_chain=16)
    with abn.Context(1) as ctx1:
        other = abn.Plan(ctx1, ped[:, :3], W, S, B, options=o)
        other.set_windows(D, p0)
        other.run()
        here = abn.Plan(gpu_ctx, ped[:, :3], W, S, B, options=o)
        here.set_windows(D, p0)
        here.run()
        want, want_cnt, want_kinds, _ = step(here, "run")      # leaves device 0 current
        cnt, ms = other.counters(), other.kernel_ms()
        assert cnt == want_cnt, (cnt, want_cnt)
        assert ms["fit_starts"] > 0 and ms["select"] > 0 and ms["fit_boot"] > 0, ms
        here.sync()                                              # device 0 current again
        assert other.last_kernels() == want_kinds
        assert_same_bytes(other.download(), want, "device 1")
        other.close()
        here.close()
