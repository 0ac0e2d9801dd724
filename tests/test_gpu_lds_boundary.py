"""Fit parity at the host's kernel decisions: LDS-resident or streamed, speculative or not, and the 160 KiB opt-in limit.

Every fit launch first decides whether a chain's pedigree fits in LDS (kLdsResidentMax = 40 KiB per workgroup,
abn_route.hpp: resident_rows) and that decision also fixes the reduction tree the oracle has to be told.  The cases
below sit one allocation step either side of each decision — the footprints differ by the smallest amount the
formula can move (two doubles per chain of the workgroup) — and check which side they landed on through
Plan.last_kernels(), so that a drift between this file's copy of the formula and the C++ fails loudly.  On every case
that runs: one tree per pedigree (abn.reduction_tree, every abn_fit_info.lanes, cost_batch), bit-equality with the
oracle at THAT tree, and results that do not depend on the size of the launch.

Generations saturate at 127 (Rust's `as i8`), so T <= 127 and K <= N bound every footprint: with 64 lanes per
chain (auto options for N > 256) the largest resident footprint, N = 1024 rows, is 30 KiB, and the LDS limit is
never the reason to stream there (N > 1024 is).  Real LDS boundaries exist with several chains per workgroup
(lanes_per_chain 8 and 16, with and without strict order), for the speculative kernel, and at the 160 KiB limit.
"""
import numpy as np
import pytest

from alphabeta_rs_amd import synthetic

# abn_route.hpp / abn_constants.hpp
KPW, WAVE = 10, 64
LDS_RESIDENT_MAX = 40 * 1024
MAX_DYN_LDS = 160 * 1024
SEL_CHUNK = 512
SPEC_OUTCOMES = 10
SPEC_COMM_DOUBLES = 8 + 2 * (SPEC_OUTCOMES * 12) + 16 + 2 * (SPEC_OUTCOMES * 3 * 12) + 16
CANON = 0x10040
ERR_INVALID_ARG = 1


def stream_tree(lanes):
    return lanes | (3 << 8)


# ------------------------------------------------------------------------------------------------ the host's arithmetic
def topology(gens):
    """(T, K, chain_stride) as build_topology computes them: i8 saturation, distinct (t0, t1-t0, t2-t0) triples."""
    g = np.clip(np.trunc(np.asarray(gens, dtype=np.float64)[:, :3]), -128, 127).astype(np.int64)
    t0, ea, eb = g[:, 0], g[:, 1] - g[:, 0], g[:, 2] - g[:, 0]
    tmax = int(max(t0.max(), ea.max(), eb.max()))
    k = len(np.unique(t0 | (ea << 8) | (eb << 16)))
    return tmax, k, KPW * (tmax + 1) + ((k + 1) & ~1) + 4


def pick_rmax(n, lanes):
    per = (n + lanes - 1) // lanes
    for r in (1, 2, 4, 8):
        if per <= r:
            return r
    return 16 if (per <= 16 and lanes == WAVE) else 0


def resident_bytes(n, k, chain_stride, lanes, strict=0):
    """route_launch's footprint of a resident workgroup (resident_extra: observations, triple list, strict terms)"""
    extra = ((n + 1) & ~1) + (((k + 1) // 2 + 1) & ~1) + (((n + 1) & ~1) if strict else 0)
    return (WAVE // lanes) * (chain_stride + extra) * 8


def streams(n, k, chain_stride, lanes, strict=0):
    return pick_rmax(n, lanes) == 0 or resident_bytes(n, k, chain_stride, lanes, strict) > LDS_RESIDENT_MAX


def spec_bytes(n, chain_stride):
    """the speculative kernel's footprint (spec_lds): three evaluation wavefronts' scratch + observations, and the exchange area"""
    return (3 * (chain_stride + ((n + 1) & ~1)) + SPEC_COMM_DOUBLES) * 8


def plan_bytes(chain_stride):
    """abn_plan_create's upper limit: one chain's scratch and a selection chunk (the streamed stride at 64 lanes is smaller)"""
    return (chain_stride + SEL_CHUNK) * 8


# ------------------------------------------------------------------------------------------------ pedigrees
def boundary_pedigree(n, tmax, k, seed=0, p0=synthetic.TRUE_P0UU):
    """n rows over exactly k distinct (t0, t1-t0, t2-t0) triples with max generation tmax (<= 127: `as i8`), each triple
    repeated to fill the rows in a seeded order; observations drawn from the synthetic model at TRUE_PARAMS."""
    assert 1 <= k <= n and 0 <= tmax <= 127
    rng = np.random.default_rng(seed)
    t0, ea, eb = np.meshgrid(np.arange(tmax + 1), np.arange(tmax + 1), np.arange(tmax + 1), indexing="ij")
    ok = (t0 + ea <= 127) & (t0 + eb <= 127)
    pool = np.stack([t0[ok], ea[ok], eb[ok]], axis=1)
    first = np.array([[0, tmax, tmax]])                        # realises T = tmax
    rest = pool[~((pool[:, 0] == 0) & (pool[:, 1] == tmax) & (pool[:, 2] == tmax))]
    tri = np.concatenate([first, rest[rng.choice(len(rest), k - 1, replace=False)]])
    uniq = np.stack([tri[:, 0], tri[:, 0] + tri[:, 1], tri[:, 0] + tri[:, 2]], axis=1).astype(np.float64)
    tid = np.arange(n) % k
    rng.shuffle(tid)
    gens = uniq[tid]
    dt = synthetic.model_divergence(uniq, p0, *synthetic.TRUE_PARAMS[:3])[tid]
    d = np.maximum(synthetic.TRUE_PARAMS[3] + dt + rng.normal(0.0, synthetic.NOISE_SD, n), 0.0)
    return np.concatenate([gens, d[:, None]], axis=1)


def lds_pair(lanes, strict=0):
    """(n, tmax, k) just under and just over kLdsResidentMax at `lanes` per chain: the largest row count that is
    LDS-resident by rows (pick_rmax > 0) and two rows fewer, with T and K chosen so that the smaller one's footprint
    is exactly the limit.  The larger one is then over by one allocation step (two observations (+ two terms) per
    chain of the workgroup)."""
    n_over = max(n for n in range(1, 1025) if pick_rmax(n, lanes) > 0)
    n_under = n_over - 2
    for k in range(n_under, 0, -1):          # as many distinct triples as the footprint allows
        for tmax in range(127, 0, -1):
            cs = KPW * (tmax + 1) + ((k + 1) & ~1) + 4
            if resident_bytes(n_under, k, cs, lanes, strict) == LDS_RESIDENT_MAX:
                assert resident_bytes(n_over, k, cs, lanes, strict) > LDS_RESIDENT_MAX
                return (n_under, tmax, k), (n_over, tmax, k)
    raise AssertionError(f"no footprint at the limit for lanes={lanes} strict={strict}")


def spec_pair():
    """(n, tmax, k) just inside / outside the speculative kernel's footprint (spec_lds): auto options, 64 lanes, up to 8 rows per lane
    (pick_rmax <= 8, N in (256, 512]); two rows more move the footprint by 3 x 2 doubles."""
    n_under = 300
    for k in range(n_under, 0, -1):
        for tmax in range(127, 0, -1):
            cs = KPW * (tmax + 1) + ((k + 1) & ~1) + 4
            if spec_bytes(n_under, cs) <= LDS_RESIDENT_MAX < spec_bytes(n_under + 2, cs):
                return (n_under, tmax, k), (n_under + 2, tmax, k)
    raise AssertionError("no speculative-kernel boundary")


def limit_k(tmax=127):
    """the largest K abn_plan_create accepts at T = tmax: (chain_stride + kSelChunk) doubles = 160 KiB exactly"""
    kp = MAX_DYN_LDS // 8 - SEL_CHUNK - 4 - KPW * (tmax + 1)
    assert plan_bytes(KPW * (tmax + 1) + kp + 4) == MAX_DYN_LDS
    return kp


# name -> (n, tmax, k, options, expected fit kernel of the pedigree's own launches: "resident" or "stream")
def boundary_cases():
    (u16, o16), (u8, o8), (us, os_) = lds_pair(16), lds_pair(8), lds_pair(16, strict=1)
    su, so = spec_pair()
    return {
        # N = 1000, K = 200, T = 350 (saturates to 127): read as in the residency window, far inside the limit at 64 lanes
        "auto64_n1000_k200": (1000, 127, 200, {}, "resident"),
        "auto64_rmax16_largest": (1024, 127, 1024, {}, "resident"),   # the largest resident footprint there is: 30 KiB
        "auto64_rmax16_rows_over": (1025, 127, 1024, {}, "stream"),
        "auto64_rmax8_largest": (512, 127, 512, {}, "resident"),
        "lanes16_under": (*u16, {"lanes_per_chain": 16}, "resident"),
        "lanes16_over": (*o16, {"lanes_per_chain": 16}, "stream"),
        "lanes8_under": (*u8, {"lanes_per_chain": 8}, "resident"),
        "lanes8_over": (*o8, {"lanes_per_chain": 8}, "stream"),
        "lanes32_rows_under": (256, 127, 256, {"lanes_per_chain": 32}, "resident"),  # 32 lanes: 30 KiB at most
        "lanes32_rows_over": (258, 127, 256, {"lanes_per_chain": 32}, "stream"),
        "strict16_under": (*us, {"lanes_per_chain": 16, "strict_order": 1}, "resident"),
        "strict16_over": (*os_, {"lanes_per_chain": 16, "strict_order": 1}, "stream"),
        "spec_under": (*su, {}, "resident"),
        "spec_over": (*so, {}, "resident"),
    }


def expected_tree(n, k, cs, opts):
    """the pedigree's reduction tree by this file's arithmetic (abn_reduction_tree)"""
    lanes = opts.get("lanes_per_chain", 0) or WAVE   # every auto case here has > 256 rows or T = 127: 64 lanes
    if opts.get("strict_order", 0) == 1:
        return 1
    if streams(n, k, cs, lanes):
        return stream_tree(lanes)
    return lanes if opts.get("lanes_per_chain", 0) else CANON


def test_boundary_pairs_sit_one_step_either_side():
    """The pairs are where the docstrings say, by this file's copy of the host formulas (no device needed)."""
    cases = boundary_cases()
    for name in ("lanes16", "lanes8", "strict16"):
        n0, t0, k0, o, _ = cases[name + "_under"]
        n1, t1, k1, _, _ = cases[name + "_over"]
        lanes, strict = o["lanes_per_chain"], o.get("strict_order", 0)
        cs = KPW * (t0 + 1) + ((k0 + 1) & ~1) + 4
        lo, hi = resident_bytes(n0, k0, cs, lanes, strict), resident_bytes(n1, k1, cs, lanes, strict)
        assert lo == LDS_RESIDENT_MAX < hi == lo + (WAVE // lanes) * 8 * (4 if strict else 2), (name, lo, hi)
        # the bound abn_api.hip used before (n / 2 + 2 doubles for the triple list) put the resident side over the limit
        old = (WAVE // lanes) * (cs + ((n0 + 1) & ~1) + n0 // 2 + 2 + (((n0 + 1) & ~1) if strict else 0)) * 8
        assert old > LDS_RESIDENT_MAX, name
    (n0, t0, k0, _, _), (n1, _, _, _, _) = cases["spec_under"], cases["spec_over"]
    cs = KPW * (t0 + 1) + ((k0 + 1) & ~1) + 4
    assert spec_bytes(n0, cs) <= LDS_RESIDENT_MAX < spec_bytes(n1, cs) == spec_bytes(n0, cs) + 48
    assert pick_rmax(n1, WAVE) == 8 and resident_bytes(n1, k0, cs, WAVE) <= LDS_RESIDENT_MAX
    # 64 lanes: even the largest resident pedigree stays far below the limit (the worked example as read: 38 512 B)
    assert resident_bytes(1024, 1024, KPW * 128 + 1024 + 4, WAVE) == 30752
    assert resident_bytes(1024, 1024, KPW * 128 + 1024 + 4, WAVE, strict=1) == 38944
    for name, (n, tmax, k, o, kind) in cases.items():
        ped = boundary_pedigree(n, tmax, k, seed=1)
        tt, kk, cs = topology(ped)
        assert (tt, kk) == (tmax, k), name
        lanes = o.get("lanes_per_chain", 0) or WAVE
        assert streams(n, k, cs, lanes, o.get("strict_order", 0)) == (kind == "stream"), name


# ------------------------------------------------------------------------------------------------ GPU
def _assert_fits_equal(best, info, want):
    assert np.array_equal(info["status"], want["status"])
    assert np.array_equal(info["iters"], want["iters"])
    assert np.array_equal(info["evals"], want["evals"])
    ok = want["status"] != 2
    assert np.array_equal(best[ok], want["best"][ok])
    assert np.array_equal(info["best_cost"][ok], want["best_cost"][ok])


def _run_plan(abn, ctx, ped, p0, S, B, o, boot_offset=0):
    plan = abn.Plan(ctx, ped[:, :3], 1, S, B, boot_offset=boot_offset, options=o)
    plan.set_windows(ped[:, 3][None, :], np.array([p0]))
    plan.run()
    out = plan.download()
    kinds = plan.last_kernels()
    plan.close()
    return out, kinds


def _check_pedigree(abn, ctx, oracle, ped, p0, opts, big_b, label, iters_a=20, iters_b=15, S=3, B=4):
    """One pedigree: the single tree, oracle parity at it, and launch-size independence of the bootstrap rows."""
    seed = 11
    o = abn.default_options(seed=seed, max_iters_start=iters_a, max_iters_boot=iters_b, **opts)
    tree = abn.reduction_tree(ped[:, :3], o)
    n = ped.shape[0]
    _, k, cs = topology(ped)
    assert tree == expected_tree(n, k, cs, opts), (label, hex(tree))
    # cost_batch: its tree is the pedigree's — except on a streamed pedigree, whose cost kernel sums lane-strided rows
    # (the stream kernels' four-row blocks exist in the fit kernels only): there it is the tree's lane count
    rng = np.random.default_rng(3)
    cand = synthetic.TRUE_PARAMS * rng.uniform(0.5, 1.5, (5, 4))
    cost = ctx.cost_batch(ped, p0, p0, 1.0, cand, options=o)
    cost_tree = tree & 0xff if (tree >> 8) & 0xff else tree
    assert np.array_equal(cost, np.array([oracle.cost(ped, p0, p0, 1.0, x, lanes=cost_tree) for x in cand])), label
    # the plan: few chains
    out, kinds = _run_plan(abn, ctx, ped, p0, S, B, o)
    assert np.all(out["info_a"]["lanes"] == tree) and np.all(out["info_b"]["lanes"] == tree), label
    s0 = abn.gen_start_simplices(seed, 0, S, ped[:, 3].max())
    fits = oracle.fit_batch(ped, p0, p0, 1.0, s0, iters_a, lanes=tree, threads=4)
    for f in ("status", "iters", "evals", "best_cost"):
        assert np.array_equal(out["info_a"][f][0], fits[f]), (label, f)
    best, info = ctx.fit_batch(ped, p0, p0, 1.0, s0, iters_a, options=o)     # abn_fit_batch: the same tree, the vertices
    assert np.all(info["lanes"] == tree), label
    _assert_fits_equal(best, info, fits)
    kk, model, pred, resid, _ = oracle.select_best(ped, p0, fits["best"])
    assert out["best_start"][0] == kk and np.array_equal(out["models"][0], model), label
    assert np.array_equal(out["pred"][0], pred) and np.array_equal(out["resid"][0], resid), label
    wraw, wres = oracle.boot_model(ped, model, pred, resid, p0, p0, 1.0, seed, 0, 0, B, max_iters=iters_b, lanes=tree,
                                   threads=4)
    assert np.array_equal(out["raw"][0], wraw), label
    assert np.array_equal(out["info_b"]["evals"][0], wres["evals"]), label
    # the same pedigree with enough bootstraps for another kernel: the rows they share are bit-identical
    big, big_kinds = _run_plan(abn, ctx, ped, p0, S, big_b, o)
    assert np.array_equal(big["models"], out["models"]), label
    assert np.array_equal(big["raw"][0, :B], out["raw"][0]), label
    assert np.array_equal(big["info_b"]["evals"][0, :B], out["info_b"]["evals"][0]), label
    assert np.all(big["info_b"]["lanes"] == tree), label
    mid, _ = _run_plan(abn, ctx, ped, p0, S, 2, o, boot_offset=big_b - 2)   # a shard at the far end of the big launch
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
    out, kinds = _run_plan(abn, gpu_ctx, ped, p0, S, B, o)
    assert kinds["starts"][0] == "stream" and kinds["boot"][0] == "stream", kinds
    assert np.all(out["info_a"]["lanes"] == tree) and np.all(out["info_b"]["lanes"] == tree)
    s0 = abn.gen_start_simplices(seed, 0, S, ped[:, 3].max())
    fits = oracle.fit_batch(ped, p0, p0, 1.0, s0, ia, lanes=tree, threads=4)
    assert np.array_equal(out["info_a"]["status"][0], fits["status"])
    assert np.array_equal(out["info_a"]["iters"][0], fits["iters"])
    assert np.array_equal(out["info_a"]["evals"][0], fits["evals"])
    kk, model, pred, resid, _ = oracle.select_best(ped, p0, fits["best"])
    assert out["best_start"][0] == kk and np.array_equal(out["models"][0], model)
    assert np.array_equal(out["pred"][0], pred) and np.array_equal(out["resid"][0], resid)
    wraw, wres = oracle.boot_model(ped, model, pred, resid, p0, p0, 1.0, seed, 0, 0, B, max_iters=ib, lanes=tree,
                                   threads=4)
    assert np.array_equal(out["raw"][0], wraw)
    assert np.array_equal(out["info_b"]["evals"][0], wres["evals"])
    cand = synthetic.TRUE_PARAMS[None, :] * np.array([[1.0, 1.0, 1.0, 1.0], [2.0, 0.5, 1.0, 0.0]])
    cost = gpu_ctx.cost_batch(ped, p0, p0, 1.0, cand, options=o)
    assert np.array_equal(cost, np.array([oracle.cost(ped, p0, p0, 1.0, x, lanes=64) for x in cand]))
    # two distinct triples more: chain_stride + kSelChunk is 16 bytes over 160 KiB
    over = boundary_pedigree(kmax + 3, 127, kmax + 2, seed=3)
    assert plan_bytes(topology(over)[2]) == MAX_DYN_LDS + 16
    with pytest.raises(abn.AbnError) as e:
        abn.Plan(gpu_ctx, over[:, :3], 1, S, B, options=o)
    assert e.value.status == ERR_INVALID_ARG
