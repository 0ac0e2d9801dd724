"""One deterministic oracle check per launchable fit-path instantiation (tests/_kernel_matrix.py: MATRIX).

Every case builds a pedigree with the N, T and K its route needs and asserts
  - the route: Plan.last_kernels() (kind and lanes), every abn_fit_info.lanes equal to the case's tree code, a non-zero
    tail_handed() on the tail hand-over cases;
  - bit-exact parity with the oracle at that tree: fits (best, best_cost, iters, evals, status) and plans (best_start,
    models, pred, resid, the raw rows, info_b); launches too large to replay on the CPU are sampled with a fixed seed,
    always with the first chain, the last one and the first chain of the last, partly filled wavefront;
  - independence from the launch: the large cases (two-pass, persistent) against the same chains run on another kernel
    (phase A: abn_fit_batch's one-pass launch; phase B: two shards through boot_offset), every row byte for byte.

test_cost_kernel_against_fifty_digits checks every abn_cost_kernel<G> against mpmath, independent of the oracle.
"""
import numpy as np
import pytest

from alphabeta_rs_amd import synthetic

import _kernel_matrix as KM
import _route_model as RM
from _parity import assert_fits_equal, check_selection_and_boot, run_plan
from _parity import sample_chains as _sample

P0 = synthetic.TRUE_P0UU
STATUS_PARKED = 4


def _check_shards(abn, ctx, ped, c, o, out, lanes, label):
    """phase B in two shards through boot_offset, each small enough for the plain resident kernel (auto lanes: possibly
    a wavefront per chain): byte-identical rows"""
    B = out["raw"].shape[1]
    half = B // 2
    for off, nb in ((0, half), (half, B - half)):
        sh, kinds, _ = run_plan(abn, ctx, ped, P0, c["S"], nb, o, boot_offset=off)
        assert kinds["boot"][0] == "resident" and kinds["boot"][1] in (lanes, 64 if c["route"] == "tail" else lanes), \
            (label, kinds)
        assert sh["raw"][0].tobytes() == out["raw"][0, off:off + nb].tobytes(), (label, off)
        assert sh["info_b"][0].tobytes() == out["info_b"][0, off:off + nb].tobytes(), (label, off)


@pytest.mark.gpu
@pytest.mark.parametrize("key", list(KM.MATRIX), ids=KM.label)
def test_instantiation_matches_oracle(abn, gpu_ctx, oracle, key):
    c = KM.MATRIX[key]
    label = KM.label(key)
    ped = KM.pedigree(c)
    o = abn.default_options(seed=c["seed"], **c["opts"])
    tree = abn.reduction_tree(ped[:, :3], o)
    assert tree == RM.expected_tree(c["n"], c["tmax"], c["k"], c["opts"]), (label, hex(tree))
    ia, ib, seed = c["opts"].get("max_iters_start"), c["opts"].get("max_iters_boot"), c["seed"]
    route = c["route"]

    if route == "cost":
        cand = synthetic.TRUE_PARAMS * np.random.default_rng(seed).uniform(0.5, 1.5, (7, 4))
        cost = gpu_ctx.cost_batch(ped, P0, P0, 1.0, cand, options=o)
        cost_tree = tree & 0xff if (tree >> 8) & 0xff else tree     # streamed: lane-strided rows (pinned as it is)
        assert np.array_equal(cost, np.array([oracle.cost(ped, P0, P0, 1.0, x, lanes=cost_tree) for x in cand])), label
        return

    lanes = key[1] if key[0] in (KM.FIT, KM.REFILL) else RM.pick_lanes(c["n"], 0, RM.chain_stride(c["tmax"], c["k"]))
    dev = gpu_ctx.device_info()
    small = dev["persistent_wavefronts_small"]
    B = KM.boot_count(c, small, dev["compute_units"])
    out, kinds, handed = run_plan(abn, gpu_ctx, ped, P0, c["S"], B, o)
    assert np.all(out["info_a"]["lanes"] == tree) and np.all(out["info_b"]["lanes"] == tree), label
    S = c["S"]
    s0 = abn.gen_start_simplices(seed, 0, S, ped[:, 3].max())

    if route in ("plan", "spec"):
        if route == "spec":
            assert kinds == {"starts": ("speculative", 64), "boot": ("speculative", 64)}, (label, kinds)
        else:
            kind = "stream" if key[2] <= 0 else "resident"
            assert kinds == {"starts": (kind, key[1]), "boot": (kind, key[1])}, (label, kinds)
        fits = oracle.fit_batch(ped, P0, P0, 1.0, s0, ia, lanes=tree, threads=4)
        assert_fits_equal(None, out["info_a"][0], fits, label)
        check_selection_and_boot(oracle, ped, P0, out, fits["best"], seed, ib, tree, label)
        if route == "plan":   # per-fit observations (abn_fit_batch, one window per fit): the same instantiation
            F = 2 * (RM.WAVE // lanes) + 3
            rng = np.random.default_rng(seed + 1)
            dobs = np.abs(ped[:, 3][None, :] * rng.uniform(0.5, 1.5, (F, ped.shape[0])))
            sf = abn.gen_start_simplices(seed, 1, F, dobs.max())
            best, info = gpu_ctx.fit_batch(ped, P0, P0, 1.0, sf, ia, dobs_rows=dobs, options=o)
            assert np.all(info["lanes"] == tree), label
            want = oracle.fit_batch(ped, P0, P0, 1.0, sf, ia, dobs_rows=dobs, lanes=tree, threads=4)
            assert_fits_equal(best, info, want, label)
        return

    if route == "twopass":
        kind_b = "stream" if key[2] <= 0 else "resident"
        assert kinds == {"starts": ("two_pass", key[1]), "boot": (kind_b, key[1])}, (label, kinds)
        ia_ = out["info_a"][0]
        assert np.all(ia_["status"] != STATUS_PARKED), label
        assert (ia_["iters"] > RM.PHASE_A_CAP).sum() > 0, label            # some chains were parked and resumed
        # the whole table against the one-pass launch of the same starts (abn_fit_batch: fit<G,R>, not two-pass)
        best, info = gpu_ctx.fit_batch(ped, P0, P0, 1.0, s0, ia, options=o)
        assert info.tobytes() == ia_.tobytes(), label
        rows = _sample(S, lanes)
        fits = oracle.fit_batch(ped, P0, P0, 1.0, s0[rows], ia, lanes=tree, threads=4)
        assert_fits_equal(best[rows], ia_[rows], fits, label)
        check_selection_and_boot(oracle, ped, P0, out, best, seed, ib, tree, label)
        return

    # persistent (explicit lanes) and tail hand-over (auto lanes: canonical tree, the tail on the speculative kernel)
    starts = ("speculative", 64) if route == "tail" else ("resident", lanes)
    assert kinds == {"starts": starts, "boot": ("persistent", lanes)}, (label, kinds)
    assert B > small * (RM.WAVE // lanes) and B % (RM.WAVE // lanes)
    if route == "tail":
        assert handed[1] > 0, (label, handed)
    fits = oracle.fit_batch(ped, P0, P0, 1.0, s0, ia, lanes=tree, threads=4)
    assert_fits_equal(None, out["info_a"][0], fits, label)
    check_selection_and_boot(oracle, ped, P0, out, fits["best"], seed, ib, tree, label, rows=_sample(B, lanes))
    _check_shards(abn, gpu_ctx, ped, c, o, out, lanes, label)


# ------------------------------------------------------------------------------------------------ cost kernel, 50 digits
def _cost_candidates():
    """alpha, beta exactly 0 or in [1e-9, 1] (1, alpha = beta, 1 - 1e-12 included; never both 0: p_uu_est is 0 / 0),
    weight in [0, 1]"""
    rng = np.random.default_rng(7)
    fixed = [(1e-9, 1e-9, 0.5), (0.0, 1e-4, 0.0), (2e-3, 0.0, 1.0), (1.0, 1.0, 0.25), (1.0, 1e-9, 0.75),
             (1 - 1e-12, 1 - 1e-12, 0.5), (1 - 1e-12, 0.3, 0.1), (0.3, 0.3, 0.9), (1e-4, 5e-4, 0.03)]
    rand = [(10 ** rng.uniform(-9, 0), 10 ** rng.uniform(-9, 0), rng.uniform(0, 1)) for _ in range(3)]
    return np.array([(a, b, w, 1e-3) for a, b, w in fixed + rand])


def _cost_pedigree(T):
    """every power 0..T in the table: (0, t, t) for t <= T, and (t, T, t) rows for the t0 powers"""
    rows = [(0, t, t) for t in range(T + 1)] + [(t, T, t) for t in sorted({0, 1, T // 2, T}) if t <= T]
    g = np.array(rows, dtype=np.float64)
    return np.concatenate([g, np.zeros((len(g), 1))], axis=1)


class _Err:
    """a value in mpmath and a bound on the absolute error of its double evaluation (running error analysis: every
    operation adds one rounding, u |result|, to the propagated errors of its operands; order and fused multiply-adds
    do not matter for the bounds used: sums of non-negative terms are bounded with gamma_n)"""

    U = None

    def __init__(self, v, e=0):
        self.v, self.e = v, e

    def __add__(self, o):
        v = self.v + o.v
        return _Err(v, self.e + o.e + self.U * abs(v))

    def __sub__(self, o):
        v = self.v - o.v
        return _Err(v, self.e + o.e + self.U * abs(v))

    def __mul__(self, o):
        v = self.v * o.v
        return _Err(v, abs(self.v) * o.e + abs(o.v) * self.e + self.e * o.e + self.U * abs(v))

    def __truediv__(self, o):
        import mpmath as mp

        v = self.v / o.v
        return _Err(v, (self.e + abs(v) * o.e) / (abs(o.v) - o.e) + self.U * abs(v)) if o.v else _Err(mp.nan, mp.inf)


_SETUP = {}


def _exact_setup(a, b, w, p_uu):
    """per candidate, at 50 digits: the power table G^0..G^127, sv0, eps_g, and p_uu_est with its running-error bound"""
    import mpmath as mp

    key = (a, b, w, p_uu)
    if key in _SETUP:
        return _SETUP[key]
    u = mp.mpf(2) ** -53
    _Err.U = u
    one = _Err(mp.mpf(1))
    A, Bt = _Err(mp.mpf(a)), _Err(mp.mpf(b))
    q = mp.mpf("0.25")
    s1, s2 = (Bt + one) - A, (A + one) - Bt
    g = [[(one - A) * (one - A), _Err(mp.mpf(2)) * (one - A) * A, A * A],
         [_Err(q) * s1 * s1, _Err(mp.mpf("0.5")) * s1 * s2, _Err(q) * s2 * s2],
         [Bt * Bt, _Err(mp.mpf(2)) * (one - Bt) * Bt, (one - Bt) * (one - Bt)]]
    G = mp.matrix([[x.v for x in r] for r in g])
    eps_g = max((x.e / x.v if x.v else mp.mpf(0)) for r in g for x in r)
    pw = [mp.eye(3)]
    for _ in range(127):
        pw.append(pw[-1] * G)
    p_mm = 1 - mp.mpf(p_uu)
    sv0 = mp.matrix([[mp.mpf(p_uu), mp.mpf(w) * p_mm, (1 - mp.mpf(w)) * p_mm]])
    num = Bt * (((one - Bt) * (one - Bt) - (one - A) * (one - A)) - one)
    sab = A + Bt
    puu = num / (sab * (((sab - one) * (sab - one)) - _Err(mp.mpf(2))))
    _SETUP[key] = (u, pw, sv0, eps_g, puu.v, puu.e)
    return _SETUP[key]


def _exact(a, b, w, p_uu, t0, t1, t2):
    """dt1t2 of one triple (src/divergence.rs:33-93) at 50 digits and its a-priori relative bound (the test's docstring)"""
    import mpmath as mp

    u, pw, sv0, eps_g, _, _ = _exact_setup(a, b, w, p_uu)
    s = sv0 * pw[t0]
    P, Q = pw[t1 - t0], pw[t2 - t0]
    d = 0
    for r in range(3):
        d += s[0, r] * (mp.mpf("0.5") * (P[r, 0] * Q[r, 1] + P[r, 1] * Q[r, 0] + P[r, 1] * Q[r, 2] + P[r, 2] * Q[r, 1])
                        + (P[r, 0] * Q[r, 2] + P[r, 2] * Q[r, 0]))
    k = t0 + (t1 - t0) + (t2 - t0)

    def gam(n):
        return n * u / (1 - n * u)

    return d, (1 + eps_g) ** k * (1 + gam(3)) ** (k + 2) * (1 + 3 * u) * (1 + gam(7)) - 1


@pytest.mark.gpu
@pytest.mark.parametrize("lanes", (8, 16, 32, 64))
def test_cost_kernel_against_fifty_digits(abn, gpu_ctx, lanes):
    """abn_cost_kernel<G> (cost_batch, want_dt / want_puu) against an mpmath evaluation of genmatrix, matrix_power,
    divergence() and p_uu_est at 50 digits — independent of the oracle, which restates the same expressions in double.

    Bound on dt.  With alpha, beta in {0} U [1e-9, 1], weight and p_uu in [0, 1], every operand of the dt computation is
    non-negative: the genmatrix entries, the power table (sums of products of them), the state vector and the six
    conditional-divergence products.  With u = 2^-53 and gamma_n = n u / (1 - n u):
      - genmatrix entry (i, j) carries a relative error eps_g, computed per candidate by running-error analysis of its
        formula (3 u for (1 - alpha)^2; the subtraction in beta + 1 - alpha is the only cancellation: alpha = 1,
        beta = 1e-9 gives eps_g ~ 4e9 u, the rounding of 1 + beta seen through a difference of 1e-9);
      - G^k, k >= 1, is a sum of non-negative products of k entries, rounded k - 1 times as 3-term dot products:
        relative error <= (1 + eps_g)^k (1 + gamma_3)^(k-1) - 1;
      - sv0 = (p_uu, w (1 - p_uu), (1 - w)(1 - p_uu)): 3 u; svt0 = sv0 G^t0: one more gamma_3;
      - dt_r: six products of entries of G^(t1-t0) and G^(t2-t0), summed (x 0.5 exact): gamma_7 covers products and sums;
      - dt = sum_r svt0_r dt_r: one more gamma_3.
    So |dt~ - dt| <= [(1 + eps_g)^k (1 + gamma_3)^(k+2) (1 + 3u)(1 + gamma_7) - 1] dt with k = t0 + (t1-t0) + (t2-t0):
    to first order (k (eps_g + 3 u) + 16 u) dt, linear in the power steps, 0 when dt = 0.  A power table off by one
    power changes dt by a relative O(alpha + beta) per step and a wrong row by O(1): far outside the bound for the
    candidates with eps_g ~ u.
    Bound on p_uu_est: its numerator (1 - beta)^2 - (1 - alpha)^2 - 1 cancels; the bound is the running-error sum of the
    intermediate magnitudes, each operation adding u |result| (mpmath, same expression tree)."""
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 50
    cand = _cost_candidates()
    p_uu = 0.75
    o = abn.default_options(lanes_per_chain=lanes)
    # 64 KiB per workgroup below 64 lanes (64/G chains' scratch): at 8 lanes these pedigrees stop at T = 91
    dts = {}
    for T in range(128):
        ped = _cost_pedigree(T)
        if lanes < 64 and (64 // lanes) * RM.topology(ped)[2] * 8 > 64 * 1024:
            assert lanes == 8 and T >= 80, T
            continue
        _, dt, puu = gpu_ctx.cost_batch(ped, p_uu, p_uu, 1.0, cand, options=o, want_dt=True, want_puu=True)
        for m, (a, b, w, _) in enumerate(cand):
            for i, t in enumerate(tuple(int(v) for v in r) for r in ped[:, :3]):
                if (m, t) not in dts:
                    dts[(m, t)] = _exact(a, b, w, p_uu, *t)
                x, r = dts[(m, t)]
                assert abs(mp.mpf(dt[m, i]) - x) <= r * x, (lanes, T, t, (a, b, w), float(dt[m, i]), float(x), float(r))
            _, _, _, _, pv, pe = _exact_setup(a, b, w, p_uu)
            assert abs(mp.mpf(puu[m]) - pv) <= pe, (lanes, T, (a, b, w), float(puu[m]), float(pv), float(pe))
