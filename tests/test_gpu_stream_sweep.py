"""abn_sweep_kernel on the GPU: a streamed chain's rows read once per Nelder-Mead iteration — the reflection, the expansion
and the contraction evaluated in one pass — must give the bits of the per-evaluation stream kernel and of the oracle at
lanes = 64 | 3 << 8, whichever branch an iteration takes, and count as the reference counts.

Row counts are placed by the sweep kernel's own loop: a lane owns blocks of 4 rows 4 (l + 64 q)..; the deep loop (R = 0,
N >= 3072) takes 12 blocks per trip (3072 rows), then pairs (512 rows), then single, possibly partial, blocks (256 rows);
the pair-loop variant (R = -1) has no deep loop.  Each lane leaves a loop when ITS next trip
would pass the last row."""
import math
import subprocess

import numpy as np
import pytest

from _parity import assert_fits_equal, synthetic_pedigree

pytestmark = pytest.mark.gpu

TREE = 64 | (3 << 8)
P0 = 0.7


def pedigree(seed, n, tmax, k_parity=None):
    """synthetic_pedigree with, on request, an odd or even number of distinct triples (one row moved to a triple that no
    row has)"""
    import _route_model as RM

    ped = synthetic_pedigree(np.random.default_rng(seed), n, tmax)
    row = 0
    while k_parity is not None and RM.topology(ped[:, :3])[1] % 2 != k_parity:
        have = {tuple(r) for r in ped[:, :3]}
        ped[row, :3] = next((t0, t1, t2) for t0 in range(tmax // 2) for t1 in range(t0, tmax + 1)
                            for t2 in range(t0, tmax + 1) if (t0, t1, t2) not in have)
        row += 1
    assert RM.topology(ped[:, :3])[0] == tmax or tmax > 100
    return ped


# ------------------------------------------------------------------------------------------------ 1. against the oracle
# (n, where its rows end in the sweep kernel's loops)
#   1100: R = -1; two pair trips (1024 rows), then single blocks for lanes 0..18 only
#   3077: R = 0; one deep trip (3072 rows), then one full block (lane 0) and a partial one (lane 1: one row)
#   3970: R = 0; one deep trip, one pair trip (to 3584); lanes 0..31 then take their last two blocks as another pair, lanes
#         32..63 one single block, and lane 32 a partial one after it (two rows): deep, pairs and a partial block all occur
#   3672: R = 0; deep trip, pair trip, then full single blocks for lanes 0..21; the higher lanes own no block in that trip
CASES = [  # n, tmax, K parity, shrink variant, no_fixed_point_skip, per-fit observations
    (1100, 12, 0, 0, 0, False), (1100, 127, 1, 1, 1, False),
    (3077, 12, 1, 1, 0, False), (3077, 127, 0, 0, 1, True),
    (3970, 12, 0, 0, 1, False), (3970, 127, 1, 1, 0, False),
    (3672, 127, 0, 0, 0, False), (3672, 12, 1, 1, 1, True),
]


@pytest.mark.parametrize("n,tmax,kpar,variant,no_skip,per_fit", CASES)
def test_fit_batch_sweep_matches_the_oracle(abn, gpu_ctx, oracle, n, tmax, kpar, variant, no_skip, per_fit):
    import _route_model as RM

    ped = pedigree(n + tmax, n, tmax, kpar)
    assert RM.topology(ped[:, :3])[1] % 2 == kpar
    F, iters, seed = 6, 300, 19
    s0 = abn.gen_start_simplices(seed, 0, F, ped[:, 3].max())
    dobs = None
    if per_fit:
        dobs = np.abs(ped[:, 3][None, :] * np.random.default_rng(n).uniform(0.7, 1.3, (F, 1)))
    o = abn.default_options(shrink_on_failed_contraction=variant, no_fixed_point_skip=no_skip)
    best, info, passes = gpu_ctx.fit_batch_sweep(ped, P0, P0, 1.0, s0, iters, dobs_rows=dobs, options=o)
    assert np.all(info["lanes"] == TREE) and abn.reduction_tree(ped[:, :3], o) == TREE
    want = oracle.fit_batch(ped, P0, P0, 1.0, s0, iters, dobs_rows=dobs, shrink_variant=variant, lanes=TREE, table=True)
    assert_fits_equal(best, info, want, (n, tmax))
    assert 5 * F <= passes <= int(want["evals"].sum())


# ------------------------------------------------------------------------------------------------ 2. every branch
def replay(oracle, ped, dobs, s0, max_iters, variant):
    """fit_impl of oracle/abn_oracle.c with its cost function, counting the branch of every iteration.  A rejected
    contraction of variant 0 leaves the simplex as it was: the remaining iterations repeat it and are counted, not run."""
    eps = np.finfo(np.float64).eps
    evals = 0

    def cost(x):
        nonlocal evals
        evals += 1
        return oracle.cost(ped, P0, P0, 1.0, np.array(x), dobs=dobs, lanes=TREE, table=True)

    def sort(v):
        for i in range(1, 5):
            if v[i][1] < v[i - 1][1]:
                tmp, hole = v[i], i
                while True:
                    v[hole] = v[hole - 1]
                    hole -= 1
                    if not (hole > 0 and tmp[1] < v[hole - 1][1]):
                        break
                v[hole] = tmp

    v = [[np.array(s0[k], dtype=np.float64), None] for k in range(5)]
    for k in range(5):
        v[k][1] = cost(v[k][0])
    sort(v)
    n = dict(refl=0, exp_kept=0, exp_rej=0, con_acc=0, con_rej=0, shrink_nan=0, shrink_textbook=0)
    it = 0
    while True:
        c = [float(x[1]) for x in v]
        c0 = ((((c[0] + c[1]) + c[2]) + c[3]) + c[4]) / 5.0
        ss = 0.0
        for ck in c:
            ss += (ck - c0) * (ck - c0)
        if math.sqrt(1.0 / (5.0 - 1.0) * ss) < eps:
            break
        if it >= max_iters:
            break
        x0 = (((v[0][0] + v[1][0]) + v[2][0]) + v[3][0]) * 0.25
        xr = x0 + (x0 - v[4][0]) * 1.0
        fr = cost(xr)
        shrink = False
        if fr < v[3][1] and fr >= v[0][1]:
            n["refl"] += 1
            v[4] = [xr, fr]
        elif fr < v[0][1]:
            xe = x0 + (xr - x0) * 2.0
            fe = cost(xe)
            n["exp_kept" if fe < fr else "exp_rej"] += 1
            v[4] = [xe, fe] if fe < fr else [xr, fr]
        elif fr >= v[3][1]:
            xc = x0 + (v[4][0] - x0) * 0.5
            fc = cost(xc)
            if fc < v[4][1]:
                n["con_acc"] += 1
                v[4] = [xc, fc]
            elif variant:
                n["shrink_textbook"] += 1
                shrink = True
            else:
                rest = max_iters - it - 1
                n["con_rej"] += 1 + rest
                evals += 2 * rest
                it += rest
        else:
            n["shrink_nan"] += 1
            shrink = True
        if shrink:
            for k in range(1, 5):
                v[k][0] = v[0][0] + (v[k][0] - v[0][0]) * 0.5
                v[k][1] = cost(v[k][0])
        sort(v)
        it += 1
    return it, evals, n


@pytest.mark.parametrize("variant,no_skip,iters", ((1, 0, 250), (0, 1, 250), (0, 0, 2000)))
def test_every_branch_matches_the_oracle_and_the_per_evaluation_kernel(abn, gpu_ctx, oracle, variant, no_skip, iters):
    """The start-simplex recipe of test_speculative_phase_a_all_branches on a streamed pedigree: windows of scaled
    observations, one of them with a NaN (every cost NaN: a shrink per iteration), and one start vertex NaN."""
    ped = pedigree(7, 1100, 12)
    N, W, S, seed = ped.shape[0], 4, 8, 91
    rng = np.random.default_rng(8)
    D = np.abs(ped[:, 3][None, :] * rng.uniform(0.7, 1.3, (W, 1)))
    D[3, 2] = np.nan
    s0 = np.concatenate([abn.gen_start_simplices(seed, w, S, float(np.fmax.reduce(D[w]))).reshape(S, 5, 4) for w in range(W)])
    s0[1, 2, :] = np.nan                          # a NaN start vertex: its cost is NaN, it never moves in the sort
    dobs = np.repeat(D, S, axis=0)
    assert dobs.shape == (W * S, N) and s0.shape == (W * S, 5, 4)
    o = abn.default_options(shrink_on_failed_contraction=variant, no_fixed_point_skip=no_skip)
    best, info, passes = gpu_ctx.fit_batch_sweep(ped, P0, P0, 1.0, s0, iters, dobs_rows=dobs, options=o)
    pbest, pinfo = gpu_ctx.fit_batch(ped, P0, P0, 1.0, s0, iters, dobs_rows=dobs, options=o)
    assert info.tobytes() == pinfo.tobytes() and np.array_equal(best, pbest, equal_nan=True)
    want = oracle.fit_batch(ped, P0, P0, 1.0, s0, iters, dobs_rows=dobs, shrink_variant=variant, lanes=TREE, table=True)
    assert_fits_equal(best, info, want)
    assert np.all(want["status"][3 * S:] == 2) and np.all(want["status"][:3 * S] != 2)
    # which branches these fits took, from the oracle: the NaN window shrinks in every iteration (5 evaluations each) ...
    nan_w = want[3 * S:]
    assert np.all(nan_w["iters"] == iters) and np.all(nan_w["evals"] == 5 + 5 * nan_w["iters"])
    # ... and the finite fits are replayed with the oracle's cost function, the replay held to the oracle's counts
    total = dict(refl=0, exp_kept=0, exp_rej=0, con_acc=0, con_rej=0, shrink_nan=0, shrink_textbook=0)
    shrinks = 0
    for f in range(3 * S):
        it, ev, n = replay(oracle, ped, dobs[f], s0[f], iters, variant)
        assert (it, ev) == (int(want["iters"][f]), int(want["evals"][f])), f
        for k in total:
            total[k] += n[k]
        shrinks += n["shrink_nan"] + n["shrink_textbook"]
    assert min(total[k] for k in ("refl", "exp_kept", "exp_rej", "con_acc")) > 0, total
    assert (total["shrink_textbook"] > 0) if variant else (total["con_rej"] > 0), total
    if variant == 0 and no_skip == 0:             # stuck fits end at the cap with the counters of the repetitions
        assert np.any((want["iters"][:3 * S] == iters) & (want["status"][:3 * S] == 1))
    assert passes <= int(want["evals"].sum())


# ------------------------------------------------------------------------------------------------ 3. C5 to termination
@pytest.fixture(scope="module")
def c5_reference(abn, oracle):
    """the oracle's answers for test_deep_pedigree_c5_fits_to_termination's shape, once for both stream modes"""
    from alphabeta_rs_amd import synthetic

    ped, p0 = synthetic.c5_pedigree()
    seed, S, B = 31, 2, 8
    s0 = abn.gen_start_simplices(seed, 0, S, ped[:, 3].max())
    fits = oracle.fit_batch(ped, p0, p0, 1.0, s0, 10000, lanes=TREE, table=True, threads=16)
    k, model, pred, resid, _ = oracle.select_best(ped, p0, fits["best"])
    wraw, wres = oracle.boot_model(ped, model, pred, resid, p0, p0, 1.0, seed, 0, 0, B, max_iters=1000, lanes=TREE,
                                   table=True, threads=16)
    return dict(ped=ped, p0=p0, seed=seed, S=S, B=B, fits=fits, k=k, model=model, pred=pred, resid=resid, raw=wraw, res=wres)


def run_plan(abn, ctx, gens, D, p0, S, B, o, sweep, ids=None):
    W = D.shape[0]
    plan = abn.Plan(ctx, gens, W, S, B, options=o)
    if ids is not None:
        plan.set_window_ids(ids)
    plan.set_stream_sweep(sweep)
    plan.set_windows(D, np.asarray(p0, dtype=np.float64).reshape(W))
    plan.run()
    out, kinds, sw, cnt = plan.download(), plan.last_kernels(), plan.stream_sweep(), plan.counters()
    plan.close()
    return out, kinds, sw, cnt


def assert_same_downloads(a, b):
    for k in ("models", "pred", "resid", "raw", "info_a", "info_b", "best_start"):
        assert a[k].tobytes() == b[k].tobytes(), k


@pytest.mark.parametrize("stream_mode", (0, 1))
def test_c5_plan_to_termination_with_the_sweep(abn, gpu_ctx, c5_reference, stream_mode):
    r = c5_reference
    ped, p0 = r["ped"], r["p0"]
    o = abn.default_options(seed=r["seed"], stream_mode=stream_mode)
    outs = {}
    for sweep in (0, 1):
        outs[sweep] = run_plan(abn, gpu_ctx, ped[:, :3], ped[:, 3][None, :], [p0], r["S"], r["B"], o, sweep)
    out, kinds, sw, _ = outs[1]
    assert kinds["starts"] == ("stream_sweep", 64) and kinds["boot"] == ("stream_sweep", 64), kinds
    assert sw["mode"] == 1 and sw["starts"] and sw["boot"] and sw["passes"] > 0, sw
    off = outs[0]
    assert off[1]["starts"][0] == "stream" and off[1]["boot"][0] == "stream", off[1]
    assert off[2] == {"mode": 0, "starts": False, "boot": False, "passes": 0}
    assert_same_downloads(out, off[0])
    assert np.all(out["info_a"]["lanes"] == TREE) and np.all(out["info_b"]["lanes"] == TREE)
    for f in ("status", "iters", "evals", "best_cost"):
        assert np.array_equal(out["info_a"][f][0], r["fits"][f]), f
    assert out["best_start"][0] == r["k"] and np.array_equal(out["models"][0], r["model"])
    assert np.array_equal(out["pred"][0], r["pred"]) and np.array_equal(out["resid"][0], r["resid"])
    assert np.array_equal(out["raw"][0], r["raw"])
    for f in ("status", "iters", "evals"):
        assert np.array_equal(out["info_b"][f][0], r["res"][f]), f
    iters = int(r["fits"]["iters"].sum()) + int(r["res"]["iters"].sum())
    assert sw["passes"] <= 5 * (r["S"] + r["B"]) + iters + 4 * iters


# ------------------------------------------------------------------------------------------------ 4. one pass per iteration
def test_one_pass_over_the_rows_per_iteration(abn, gpu_ctx, oracle):
    """no_fixed_point_skip = 1: every iteration is executed.  Seed 23 is one at which no fit shrinks (finite data: a
    shrink needs a NaN reflection), shown below from the oracle: the starts replayed, the bootstraps traced."""
    ped = pedigree(3, 3077, 12)
    seed, S, B, ia, ib = 23, 3, 6, 60, 40
    o = abn.default_options(seed=seed, no_fixed_point_skip=1, max_iters_start=ia, max_iters_boot=ib)
    out, kinds, sw, cnt = run_plan(abn, gpu_ctx, ped[:, :3], ped[:, 3][None, :], [P0], S, B, o, 1)
    assert kinds["starts"][0] == "stream_sweep" and kinds["boot"][0] == "stream_sweep" and np.all(np.isfinite(ped))
    s0 = abn.gen_start_simplices(seed, 0, S, ped[:, 3].max())
    fits = oracle.fit_batch(ped, P0, P0, 1.0, s0, ia, lanes=TREE, table=True)
    k, model, pred, resid, _ = oracle.select_best(ped, P0, fits["best"])
    wraw, wres, trace = oracle.boot_model_trace(ped, model, pred, resid, P0, P0, 1.0, seed, 0, 0, B, max_iters=ib, lanes=TREE,
                                                table=True)
    for f in ("status", "iters", "evals"):
        assert np.array_equal(out["info_a"][f][0], fits[f]) and np.array_equal(out["info_b"][f][0], wres[f]), f
    assert np.array_equal(out["raw"][0], wraw)
    for f in range(S):                                              # no start shrank ...
        it, ev, n = replay(oracle, ped, None, s0.reshape(S, 5, 4)[f], ia, 0)
        assert (it, ev) == (int(fits["iters"][f]), int(fits["evals"][f])) and n["shrink_nan"] == n["shrink_textbook"] == 0
    for b in range(B):                                              # ... and no bootstrap did
        assert not np.any(trace[b, :wres["iters"][b]] == 4), b
    iters = int(fits["iters"].sum()) + int(wres["iters"].sum())
    evals = int(fits["evals"].sum()) + int(wres["evals"].sum())
    assert sw["passes"] == 5 * (S + B) + iters
    assert sw["passes"] < evals == cnt["evals"]
    assert cnt["evals_skipped"] == 0


# ------------------------------------------------------------------------------------------------ 5. several windows
@pytest.mark.parametrize("stream_mode", (0, 1))
def test_multi_window_plan_with_window_ids(abn, gpu_ctx, oracle, stream_mode):
    ped = pedigree(11, 1100, 12)
    W, S, B, seed = 3, 3, 5, 77
    ids = np.array([7, 2, 11], dtype=np.uint32)
    rng = np.random.default_rng(4)
    D = np.abs(ped[:, 3][None, :] * rng.uniform(0.8, 1.25, (W, 1)))
    p0 = rng.uniform(0.6, 0.8, W)
    o = abn.default_options(seed=seed, max_iters_start=50, max_iters_boot=30, stream_mode=stream_mode)
    on, kinds, sw, _ = run_plan(abn, gpu_ctx, ped[:, :3], D, p0, S, B, o, 1, ids)
    off, koff, swoff, _ = run_plan(abn, gpu_ctx, ped[:, :3], D, p0, S, B, o, 0, ids)
    assert kinds["starts"][0] == kinds["boot"][0] == "stream_sweep" and sw["starts"] and sw["boot"], (kinds, sw)
    assert koff["starts"][0] == koff["boot"][0] == "stream" and not swoff["starts"] and not swoff["boot"]
    assert_same_downloads(on, off)
    for w in range(W):
        pw = np.concatenate([ped[:, :3], D[w][:, None]], axis=1)
        s0 = abn.gen_start_simplices(seed, int(ids[w]), S, D[w].max())
        fits = oracle.fit_batch(pw, p0[w], p0[w], 1.0, s0, 50, lanes=TREE, table=True)
        for f in ("status", "iters", "evals"):
            assert np.array_equal(on["info_a"][f][w], fits[f]), (w, f)
        k, model, pred, resid, _ = oracle.select_best(pw, p0[w], fits["best"])
        assert on["best_start"][w] == k and np.array_equal(on["models"][w], model)
        assert np.array_equal(on["pred"][w], pred) and np.array_equal(on["resid"][w], resid)
        wraw, wres = oracle.boot_model(pw, model, pred, resid, p0[w], p0[w], 1.0, seed, int(ids[w]), 0, B, max_iters=30,
                                       lanes=TREE, table=True)
        assert np.array_equal(on["raw"][w], wraw), w
        for f in ("status", "iters", "evals"):
            assert np.array_equal(on["info_b"][f][w], wres[f]), (w, f)


def test_multi_device_handle_forwards_the_switch(abn, gpu_ctx):
    """MultiPlan on one device: with the switch on, the downloads are those of a Plan that reports the sweep kernel for both
    phases, byte for byte, and those of the handle with the switch off; another mode is refused with the handle's error."""
    ped = pedigree(11, 1100, 12)
    W, S, B, seed = 3, 3, 5, 77
    ids = np.array([7, 2, 11], dtype=np.uint32)
    rng = np.random.default_rng(4)
    D = np.abs(ped[:, 3][None, :] * rng.uniform(0.8, 1.25, (W, 1)))
    p0 = rng.uniform(0.6, 0.8, W)
    o = abn.default_options(seed=seed, max_iters_start=50, max_iters_boot=30)
    want, kinds, sw, _ = run_plan(abn, gpu_ctx, ped[:, :3], D, p0, S, B, o, 1, ids)
    assert kinds["starts"][0] == kinds["boot"][0] == "stream_sweep" and sw["starts"] and sw["boot"]
    outs = []
    for mode in (1, 0):
        m = abn.MultiPlan([0], ped[:, :3], W, S, B, options=o)
        m.set_window_ids(ids)
        with pytest.raises(abn.AbnError) as err:
            m.set_stream_sweep(2)
        assert err.value.status == 1 and "stream sweep" in str(err.value)
        m.set_stream_sweep(mode)
        m.set_windows(D, p0)
        m.run()
        outs.append(m.download())
        m.close()
        assert_same_downloads(outs[-1], want)


# ------------------------------------------------------------------------------------------------ 6. fallbacks
def test_launches_the_sweep_does_not_take_run_what_they_ran(abn, gpu_ctx):
    from alphabeta_rs_amd import synthetic

    c3, p0 = synthetic.c3_pedigree()
    big = pedigree(5, 1100, 12)
    for name, ped, p, S, B, opts in (
            ("resident", c3, p0, 6, 12, dict(seed=3)),
            ("strict", big, P0, 2, 3, dict(seed=3, strict_order=1, max_iters_start=30, max_iters_boot=20))):
        o = abn.default_options(**opts)
        on, kon, swon, _ = run_plan(abn, gpu_ctx, ped[:, :3], ped[:, 3][None, :], [p], S, B, o, 1)
        off, koff, _, _ = run_plan(abn, gpu_ctx, ped[:, :3], ped[:, 3][None, :], [p], S, B, o, 0)
        assert kon == koff and "stream_sweep" not in (kon["starts"][0], kon["boot"][0]), (name, kon, koff)
        assert swon == {"mode": 1, "starts": False, "boot": False, "passes": 0}, (name, swon)
        assert_same_downloads(on, off)
    assert koff["starts"][0] == "stream" and int(off["info_a"]["lanes"][0, 0]) == 1          # the strict plan streams
    s0 = abn.gen_start_simplices(3, 0, 4, c3[:, 3].max())
    with pytest.raises(abn.AbnError) as err:
        gpu_ctx.fit_batch_sweep(c3, p0, p0, 1.0, s0, 50)
    assert err.value.status == 1 and "sweep" in str(err.value)
    for o in (abn.default_options(strict_order=1), abn.default_options(lanes_per_chain=16)):
        with pytest.raises(abn.AbnError) as err:
            gpu_ctx.fit_batch_sweep(big, P0, P0, 1.0, abn.gen_start_simplices(3, 0, 2, big[:, 3].max()), 20, options=o)
        assert err.value.status == 1
    plan = abn.Plan(gpu_ctx, big[:, :3], 1, 2, 2)
    with pytest.raises(abn.AbnError) as err:
        plan.set_stream_sweep(2)
    assert err.value.status == 1 and plan.stream_sweep()["mode"] == 0
    plan.close()


# ------------------------------------------------------------------------------------------------ 7. the command-line tool
def test_alphabeta_cli_writes_the_same_files_with_the_switch(abn, gpu_ctx, tmp_path):
    from alphabeta_rs_amd import build as B

    cli = str(B.build_host())
    ped = pedigree(13, 1100, 12)
    f = tmp_path / "pedigree_in.txt"
    f.write_text("time0\ttime1\ttime2\tD.value\n" + "".join(f"{int(a)}\t{int(b)}\t{int(c)}\t{float(d)!r}\n" for a, b, c, d in ped))
    got = {}
    for name, flag in (("off", []), ("on", ["--stream-sweep"])):
        out = tmp_path / name
        out.mkdir()
        r = subprocess.run([cli, "-i", "20", "--pedigree", str(f), "--p0uu", str(P0), "--seed", "9", "-o", str(out), *flag],
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        got[name] = ((out / "raw.npy").read_bytes(), (out / "analysis.txt").read_text())
    assert np.load(tmp_path / "on" / "raw.npy").shape == (20, 7)
    assert got["on"] == got["off"]
    help_ = subprocess.run([cli, "--help"], capture_output=True, text=True, timeout=60).stdout
    assert "--stream-sweep" in help_


def test_metaprofile_cli_writes_the_same_files_with_the_switch(abn, gpu_ctx, tmp_path):
    """`metaprofile_alphabeta --stream-sweep` on window directories of the bundled (LDS-resident) pedigree: the flag goes
    through the batched plans' handle and, no launch of theirs streaming, changes no byte of results.txt or raw.npy"""
    import shutil
    from pathlib import Path

    from alphabeta_rs_amd import build as B

    B.build_host()
    gold = Path(__file__).resolve().parent / "golden"
    got = {}
    for name, flag in (("off", []), ("on", ["--stream-sweep"])):
        out = tmp_path / name
        for r in ("upstream", "gene", "downstream"):
            for w in (0, 50):
                d = out / r / str(w)
                d.mkdir(parents=True)
                shutil.copy(gold / "data" / "edgelist.txt", d / "edgelist.txt")
                shutil.copy(gold / "data" / "nodelist.txt", d / "nodelist.txt")
        r = subprocess.run([str(B.META_CLI), "-o", str(out), "--name", "t", "-s", "50", "--iterations", "8", "--seed", "123",
                            *flag], capture_output=True, text=True, cwd=str(gold), timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        got[name] = ((out / "results.txt").read_text(), (out / "raw.npy").read_bytes())
    assert np.load(tmp_path / "on" / "raw.npy").shape == (8, 7, 6)
    assert got["on"] == got["off"]
    help_ = subprocess.run([str(B.META_CLI), "--help"], capture_output=True, text=True, timeout=60).stdout
    assert "--stream-sweep" in help_
