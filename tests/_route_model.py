"""The tests' model of the host's fit launch policy: an independent Python restatement of csrc/abn_route.hpp and the
constants of abn_constants.hpp / abn_common.hpp it decides with.

Plain data, integer arithmetic and numpy: importable without a device and without the product library.  It stays a
restatement — it reads neither abn_route.hpp nor abn_constants.hpp and calls neither abh_route_* nor
abn.reduction_tree — so that a drift between it and the C++ fails the tests that hold the two side by side
(tests/test_kernel_matrix_census.py on the CPU, Plan.last_kernels() and abn_fit_info.lanes on the GPU).

What restates what:
  topology, chain_stride                      build_topology (i8 saturation, distinct triples, a chain's scratch doubles)
  pick_lanes, strict_of                       pick_lanes; resolve_for (auto options: serial sums up to 16 rows)
  pick_rmax, resident_bytes, streams          resident_rows / resident_extra / route_launch's LDS-residency decision
  spec_bytes, spec_fits                       spec_lds; route_pedigree's spec_ok
  plan_bytes, limit_k                         abn_plan_create's 160 KiB opt-in limit
  stream_tree, expected_tree                  abn_reduction_tree (the code every abn_fit_info.lanes reports)
  fit_rmax                                    the RMAX template argument route_launch picks
boundary_pedigree builds a pedigree with a given (N, T, K); lds_pair, spec_pair and boundary_cases place pedigrees one
allocation step either side of each decision (tests/test_gpu_lds_boundary.py).
"""
import numpy as np

from alphabeta_rs_amd import synthetic

# abn_route.hpp / abn_constants.hpp
KPW, WAVE = 10, 64
LDS_RESIDENT_MAX = 40 * 1024
MAX_DYN_LDS = 160 * 1024
SEL_CHUNK = 512
SPEC_OUTCOMES = 10
SPEC_COMM_DOUBLES = 8 + 2 * (SPEC_OUTCOMES * 12) + 16 + 2 * (SPEC_OUTCOMES * 3 * 12) + 16
CANON = 0x10040                           # the tree of every LDS-resident pedigree: 64 accumulators, high lane bits first
ERR_INVALID_ARG = 1
STREAM_BLOCKS, STREAM_VEC = 6, 4          # abn_common.hpp: kStreamBlocks, kStreamVec
DEEP_ROWS = 2 * STREAM_BLOCKS * STREAM_VEC  # route_launch: N >= 48 G rows take the deep stream loop (RMAX 0), fewer -1
LDS_TARGET_PER_BLOCK = 20 * 1024          # pick_lanes' widening target
SERIAL_SUM_MAX_ROWS = 16                  # resolve_for: auto options sum up to 16 rows serially
PHASE_A_CAP = 1000                        # kPhaseACap: first-pass iteration cap of the two-pass phase A
TWO_PASS_CHAINS = 4096                    # abn_plan_create: two passes above 4096 start chains


def stream_tree(lanes):
    return lanes | (3 << 8)


# ------------------------------------------------------------------------------------------------ the host's arithmetic
def chain_stride(tmax, k):
    return KPW * (tmax + 1) + ((k + 1) & ~1) + 4


def topology(gens):
    """(T, K, chain_stride) as build_topology computes them: i8 saturation, distinct (t0, t1-t0, t2-t0) triples."""
    g = np.clip(np.trunc(np.asarray(gens, dtype=np.float64)[:, :3]), -128, 127).astype(np.int64)
    t0, ea, eb = g[:, 0], g[:, 1] - g[:, 0], g[:, 2] - g[:, 0]
    tmax = int(max(t0.max(), ea.max(), eb.max()))
    k = len(np.unique(t0 | (ea << 8) | (eb << 16)))
    return tmax, k, chain_stride(tmax, k)


def pool_size(tmax):
    """distinct (t0, t1-t0, t2-t0) triples with max generation <= tmax (t1, t2 <= 127)"""
    t = np.arange(tmax + 1)
    t0, ea, eb = np.meshgrid(t, t, t, indexing="ij")
    return int(((t0 + ea <= 127) & (t0 + eb <= 127)).sum())


def pick_lanes(n, requested, cs):
    """abn_route.hpp: pick_lanes (rows first, then widened until 64/G chains' scratch + observations fit 20 KiB)"""
    if requested:
        return requested
    g = 8 if n <= 32 else 16 if n <= 128 else 32 if n <= 256 else WAVE
    while g < WAVE and (WAVE // g) * (cs + n) * 8 > LDS_TARGET_PER_BLOCK:
        g *= 2
    return g


def strict_of(n, opts):
    """resolve_for: strict_order 0 with auto lanes is serial up to 16 rows"""
    s = opts.get("strict_order", 0)
    return 1 if s == 1 or (s == 0 and not opts.get("lanes_per_chain", 0) and n <= SERIAL_SUM_MAX_ROWS) else 0


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


def expected_tree(n, tmax, k, opts):
    """abn_reduction_tree by this restatement"""
    cs = chain_stride(tmax, k)
    lanes = pick_lanes(n, opts.get("lanes_per_chain", 0), cs)
    if strict_of(n, opts):
        return 1
    if streams(n, k, cs, lanes):
        return stream_tree(lanes)
    return lanes if opts.get("lanes_per_chain", 0) else CANON


def fit_rmax(n, k, tmax, lanes, strict):
    """the RMAX template argument route_launch (abn_route.hpp) picks: resident R, or 0 / -1 streamed (strict order streams with 0)"""
    cs = chain_stride(tmax, k)
    if not streams(n, k, cs, lanes, strict):
        return pick_rmax(n, lanes)
    return 0 if strict or n >= DEEP_ROWS * lanes else -1


def spec_fits(n, tmax, k, strict):
    """route_pedigree's spec_ok for a resident pedigree at auto lanes (canonical tree or strict order)"""
    cs = chain_stride(tmax, k)
    r = pick_rmax(n, WAVE)
    if r == 0 or r > 8 or streams(n, k, cs, WAVE, strict):
        return False
    np_ = ((n + 1) & ~1) * (2 if strict else 1)
    return (3 * (cs + np_) + SPEC_COMM_DOUBLES) * 8 <= LDS_RESIDENT_MAX


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
            cs = chain_stride(tmax, k)
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
            cs = chain_stride(tmax, k)
            if spec_bytes(n_under, cs) <= LDS_RESIDENT_MAX < spec_bytes(n_under + 2, cs):
                return (n_under, tmax, k), (n_under + 2, tmax, k)
    raise AssertionError("no speculative-kernel boundary")


def limit_k(tmax=127):
    """the largest K abn_plan_create accepts at T = tmax: (chain_stride + kSelChunk) doubles = 160 KiB exactly"""
    kp = MAX_DYN_LDS // 8 - SEL_CHUNK - 4 - KPW * (tmax + 1)
    assert plan_bytes(chain_stride(tmax, kp)) == MAX_DYN_LDS
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
