"""Fit parity at the host's kernel decisions: LDS-resident or streamed, speculative or not, and the 160 KiB opt-in limit.

Every fit launch first decides whether a chain's pedigree fits in LDS (kLdsResidentMax = 40 KiB per workgroup,
abn_route.hpp: resident_rows) and that decision also fixes the reduction tree the oracle has to be told.  The cases
below sit one allocation step either side of each decision — the footprints differ by the smallest amount the
formula can move (two doubles per chain of the workgroup) — and check which side they landed on through
Plan.last_kernels(), so that a drift between the tests' copy of the formula (tests/_route_model.py) and the C++ fails
loudly.  On every case that runs: one tree per pedigree (abn.reduction_tree, every abn_fit_info.lanes, cost_batch),
bit-equality with the oracle at THAT tree, and results that do not depend on the size of the launch.

Generations saturate at 127 (Rust's `as i8`), so T <= 127 and K <= N bound every footprint: with 64 lanes per
chain (auto options for N > 256) the largest resident footprint, N = 1024 rows, is 30 KiB, and the LDS limit is
never the reason to stream there (N > 1024 is).  Real LDS boundaries exist with several chains per workgroup
(lanes_per_chain 8 and 16, with and without strict order), for the speculative kernel, and at the 160 KiB limit.
"""
import numpy as np
import pytest

from alphabeta_rs_amd import synthetic

from _parity import assert_fits_equal, check_selection_and_boot, run_plan
from _route_model import (ERR_INVALID_ARG, LDS_RESIDENT_MAX, MAX_DYN_LDS, WAVE, boundary_cases, boundary_pedigree,
                          chain_stride, expected_tree, limit_k, pick_rmax, plan_bytes, resident_bytes, spec_bytes,
                          stream_tree, streams, topology)


def test_boundary_pairs_sit_one_step_either_side():
    """The pairs are where the docstrings say, by the tests' copy of the host formulas (no device needed)."""
    cases = boundary_cases()
    for name in ("lanes16", "lanes8", "strict16"):
        n0, t0, k0, o, _ = cases[name + "_under"]
        n1, t1, k1, _, _ = cases[name + "_over"]
        lanes, strict = o["lanes_per_chain"], o.get("strict_order", 0)
        cs = chain_stride(t0, k0)
        lo, hi = resident_bytes(n0, k0, cs, lanes, strict), resident_bytes(n1, k1, cs, lanes, strict)
        assert lo == LDS_RESIDENT_MAX < hi == lo + (WAVE // lanes) * 8 * (4 if strict else 2), (name, lo, hi)
        # the bound abn_api.hip used before (n / 2 + 2 doubles for the triple list) put the resident side over the limit
        old = (WAVE // lanes) * (cs + ((n0 + 1) & ~1) + n0 // 2 + 2 + (((n0 + 1) & ~1) if strict else 0)) * 8
        assert old > LDS_RESIDENT_MAX, name
    (n0, t0, k0, _, _), (n1, _, _, _, _) = cases["spec_under"], cases["spec_over"]
    cs = chain_stride(t0, k0)
    assert spec_bytes(n0, cs) <= LDS_RESIDENT_MAX < spec_bytes(n1, cs) == spec_bytes(n0, cs) + 48
    assert pick_rmax(n1, WAVE) == 8 and resident_bytes(n1, k0, cs, WAVE) <= LDS_RESIDENT_MAX
    # 64 lanes: even the largest resident pedigree stays far below the limit (the worked example as read: 38 512 B)
    assert resident_bytes(1024, 1024, chain_stride(127, 1024), WAVE) == 30752
    assert resident_bytes(1024, 1024, chain_stride(127, 1024), WAVE, strict=1) == 38944
    for name, (n, tmax, k, o, kind) in cases.items():
        ped = boundary_pedigree(n, tmax, k, seed=1)
        tt, kk, cs = topology(ped)
        assert (tt, kk) == (tmax, k), name
        lanes = o.get("lanes_per_chain", 0) or WAVE
        assert streams(n, k, cs, lanes, o.get("strict_order", 0)) == (kind == "stream"), name


# ------------------------------------------------------------------------------------------------ GPU
def _check_pedigree(abn, ctx, oracle, ped, p0, opts, big_b, label, iters_a=20, iters_b=15, S=3, B=4):
    """One pedigree: the single tree, oracle parity at it, and launch-size independence of the bootstrap rows."""
    seed = 11
    o = abn.default_options(seed=seed, max_iters_start=iters_a, max_iters_boot=iters_b, **opts)
    tree = abn.reduction_tree(ped[:, :3], o)
    n = ped.shape[0]
    tmax, k, _ = topology(ped)
    assert tree == expected_tree(n, tmax, k, opts), (label, hex(tree))
    # cost_batch: its tree is the pedigree's — except on a streamed pedigree, whose cost kernel sums lane-strided rows
    # (the stream kernels' four-row blocks exist in the fit kernels only): there it is the tree's lane count
    rng = np.random.default_rng(3)
    cand = synthetic.TRUE_PARAMS * rng.uniform(0.5, 1.5, (5, 4))
    cost = ctx.cost_batch(ped, p0, p0, 1.0, cand, options=o)
    cost_tree = tree & 0xff if (tree >> 8) & 0xff else tree
    assert np.array_equal(cost, np.array([oracle.cost(ped, p0, p0, 1.0, x, lanes=cost_tree) for x in cand])), label
    # the plan: few chains
    out, kinds, _ = run_plan(abn, ctx, ped, p0, S, B, o)
    assert np.all(out["info_a"]["lanes"] == tree) and np.all(out["info_b"]["lanes"] == tree), label
    s0 = abn.gen_start_simplices(seed, 0, S, ped[:, 3].max())
    fits = oracle.fit_batch(ped, p0, p0, 1.0, s0, iters_a, lanes=tree, threads=4)
    for f in ("status", "iters", "evals", "best_cost"):
        assert np.array_equal(out["info_a"][f][0], fits[f]), (label, f)
    best, info = ctx.fit_batch(ped, p0, p0, 1.0, s0, iters_a, options=o)     # abn_fit_batch: the same tree, the vertices
    assert np.all(info["lanes"] == tree), label
    assert_fits_equal(best, info, fits, label)
    assert not np.isnan(out["raw"]).any(), label                    # the replay below lets NaN meet NaN: none here
    check_selection_and_boot(oracle, ped, p0, out, fits["best"], seed, iters_b, tree, label, info_fields=("evals",))
    # the same pedigree with enough bootstraps for another kernel: the rows they share are bit-identical
    big, big_kinds, _ = run_plan(abn, ctx, ped, p0, S, big_b, o)
    assert np.array_equal(big["models"], out["models"]), label
    assert np.array_equal(big["raw"][0, :B], out["raw"][0]), label
    assert np.array_equal(big["info_b"]["evals"][0, :B], out["info_b"]["evals"][0]), label
    assert np.all(big["info_b"]["lanes"] == tree), label
    mid, _, _ = run_plan(abn, ctx, ped, p0, S, 2, o, boot_offset=big_b - 2)   # a shard at the far end of the big launch
    assert np.array_equal(mid["raw"][0], big["raw"][0, big_b - 2:]), label
    print(f"BOUNDARY {label}: N={n} K={k} tree={tree:#x} starts={kinds['starts']} boot={kinds['boot']} "
          f"boot[B={big_b}]={big_kinds['boot']}")
    return kinds, big_kinds


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(boundary_cases()))
def test_lds_boundary_pair_matches_oracle_at_the_reported_tree(abn, gpu_ctx, oracle, name):
    n, tmax, k, opts, kind = boundary_cases()[name]
    ped = boundary_pedigree(n, tmax, k, seed=7)
    p0 = synthetic.TRUE_P0UU
    lanes = opts.get("lanes_per_chain", 0)
    # big enough for the persistent kernel with several chains per wavefront (> 2048 workgroups), else for the plain
    # resident / stream kernel instead of the speculative one
    big_b = 8200 * 2 if lanes in (8, 16) else 1600
    kinds, big_kinds = _check_pedigree(abn, gpu_ctx, oracle, ped, p0, opts, big_b, name)
    if kind == "stream":
        assert kinds["starts"][0] == "stream" and kinds["boot"][0] == "stream", kinds
        assert big_kinds["boot"][0] == "stream", big_kinds
    elif name == "spec_under":
        assert kinds["starts"] == ("speculative", 64) and kinds["boot"] == ("speculative", 64), kinds
    elif name == "spec_over" or not lanes:
        # speculative kernel ruled out: one wavefront per chain (N > 256: 64 lanes is also the packed width)
        assert kinds["starts"] == ("resident", 64) and kinds["boot"] == ("resident", 64), kinds
    else:
        assert kinds["starts"] == ("resident", lanes) and kinds["boot"] == ("resident", lanes), kinds
        # several chains per wavefront and > 2048 workgroups: the persistent kernel (strict order has no such variant)
        persistent = lanes in (8, 16) and not opts.get("strict_order", 0)
        assert big_kinds["boot"] == ("persistent" if persistent else "resident", lanes), big_kinds


@pytest.mark.gpu
def test_upper_lds_limit_runs_just_under_and_is_refused_just_over(abn, gpu_ctx, oracle):
    """abn_plan_create's 160 KiB limit, T = 127: K = limit_k() distinct triples (chain_stride + kSelChunk doubles =
    160 KiB exactly) builds, runs (streamed) and matches the oracle; two triples more are refused when the Plan is
    created, with ABN_ERR_INVALID_ARG, not at run()."""
    kmax = limit_k()
    p0 = synthetic.TRUE_P0UU
    ped = boundary_pedigree(kmax + 1, 127, kmax, seed=3)
    _, k, cs = topology(ped)
    assert k == kmax and plan_bytes(cs) == MAX_DYN_LDS
    seed, S, B, ia, ib = 5, 2, 3, 20, 15
    o = abn.default_options(seed=seed, max_iters_start=ia, max_iters_boot=ib)
    tree = abn.reduction_tree(ped[:, :3], o)
    assert tree == stream_tree(64)
    out, kinds, _ = run_plan(abn, gpu_ctx, ped, p0, S, B, o)
    assert kinds["starts"][0] == "stream" and kinds["boot"][0] == "stream", kinds
    assert np.all(out["info_a"]["lanes"] == tree) and np.all(out["info_b"]["lanes"] == tree)
    s0 = abn.gen_start_simplices(seed, 0, S, ped[:, 3].max())
    fits = oracle.fit_batch(ped, p0, p0, 1.0, s0, ia, lanes=tree, threads=4)
    assert np.array_equal(out["info_a"]["status"][0], fits["status"])
    assert np.array_equal(out["info_a"]["iters"][0], fits["iters"])
    assert np.array_equal(out["info_a"]["evals"][0], fits["evals"])
    assert not np.isnan(out["raw"]).any()                           # the replay below lets NaN meet NaN: none here
    check_selection_and_boot(oracle, ped, p0, out, fits["best"], seed, ib, tree, info_fields=("evals",))
    cand = synthetic.TRUE_PARAMS[None, :] * np.array([[1.0, 1.0, 1.0, 1.0], [2.0, 0.5, 1.0, 0.0]])
    cost = gpu_ctx.cost_batch(ped, p0, p0, 1.0, cand, options=o)
    assert np.array_equal(cost, np.array([oracle.cost(ped, p0, p0, 1.0, x, lanes=64) for x in cand]))
    # two distinct triples more: chain_stride + kSelChunk is 16 bytes over 160 KiB
    over = boundary_pedigree(kmax + 3, 127, kmax + 2, seed=3)
    assert plan_bytes(topology(over)[2]) == MAX_DYN_LDS + 16
    with pytest.raises(abn.AbnError) as e:
        abn.Plan(gpu_ctx, over[:, :3], 1, S, B, options=o)
    assert e.value.status == ERR_INVALID_ARG
