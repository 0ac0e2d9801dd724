"""The observation step, the state census and the replicate study on the device (abn_sim_observe*, abn_packed_census_windows*,
abn_sim_study through alphabeta_rs_amd.simulate and alphabeta_rs_amd.census) against the numpy model of
tests/_sim_obs_model.py, bit for bit: the sizes around the dword, the 64-byte step, a wavefront and a workgroup and one past
the launch's first grid-stride trip; thresholds at the ends of their range, equal pairs and planted ties of the high word;
in place and out of place; the law's properties; window edges around the dword, the super-step and the chunk; the study's
replicates as the columns of one simulation, its statistics, and its fit through a Plan."""
import ctypes as C

import numpy as np
import pytest

import _sim_model as M
import _sim_obs_model as O
from alphabeta_rs_amd import census as Cn
from alphabeta_rs_amd import simulate as S

pytestmark = pytest.mark.gpu
SEED = 0x9E3779B97F4A7C15
RATES = (2e-3, 5e-3, 0.7, 0.3)
STUDY_L, STUDY_R, STUDY_SEED = 50_001, 5, 20260101       # replicate edges fall inside dwords
CUTS = (0, 1, 15, 16, 17, 255, 256, 257, 32_767, 32_768, 32_769)


@pytest.fixture(scope="module")
def hip():
    h = C.CDLL("libamdhip64.so")        # the HIP runtime the product library already holds
    h.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    h.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    h.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
    h.hipFree.argtypes = [C.c_void_p]
    return h


def truth(rng, rows, L, with_3=True):
    return rng.integers(0, 4 if with_3 else 3, size=(rows, L), dtype=np.uint8)


# ------------------------------------------------------------------------------------------------ the observation
@pytest.mark.parametrize("rows", (1, 8))
def test_observe_equals_the_model(gpu_ctx, rows):
    rng = np.random.default_rng(30 + rows)
    nodes = [(5 * r + 2) % 11 for r in range(rows)]                           # not the identity
    for L in M.SIZES:
        packed = M.pack(truth(rng, rows, L))
        for othr in (O.obs_thresholds(*O.noise(0.05, 0.1)), O.random_othr(rng)):
            got = S.observe(gpu_ctx, SEED, packed, nodes, O.as_array(othr), L)
            assert np.array_equal(got, O.observe(SEED, packed, nodes, othr, L)), (L, othr)
    assert np.array_equal(got, S.observe_host(SEED, packed, nodes, O.as_array(othr), L))
    assert S.observe(gpu_ctx, SEED, np.zeros((rows, 0), dtype=np.uint8), nodes, O.as_array(othr), 0).shape == (rows, 0)


def test_in_place_out_of_place_and_the_stride(abn, gpu_ctx, hip):
    rng = np.random.default_rng(33)
    rows, L = 3, 4097
    nodes, othr = [4, 0, 9], O.random_othr(rng)
    least = M.row_stride(L)
    fields = truth(rng, rows, L)
    fields[1, 100:140] = 3                                                      # planted inside a row
    packed = M.pack(fields, stride=least + 64, fill=0x5A)
    want = O.observe(SEED, packed, nodes, othr, L, stride=least + 64, fill=0x5A)
    assert (O.unpack(want, L)[fields == 3] == 3).all() and (O.unpack(want, L)[fields < 3] < 4).all()
    bufs = [C.c_void_p(), C.c_void_p()]
    for ptr in bufs:
        assert hip.hipMalloc(C.byref(ptr), packed.nbytes) == 0
    try:
        def up(ptr, a):
            assert hip.hipMemcpy(ptr, a.ctypes.data, a.nbytes, 1) == 0

        def down(ptr):
            host = np.zeros_like(packed)
            assert hip.hipMemcpy(host.ctypes.data, ptr, host.nbytes, 2) == 0
            return host

        up(bufs[0], packed)
        assert hip.hipMemset(bufs[1], 0x5A, packed.nbytes) == 0
        ms = S.observe_dev(gpu_ctx, SEED, nodes, O.as_array(othr), L, bufs[0].value, least + 64, bufs[1].value, least + 64)
        assert ms > 0
        out_of_place = down(bufs[1])
        assert np.array_equal(out_of_place, want) and np.array_equal(down(bufs[0]), packed)
        S.observe_dev(gpu_ctx, SEED, nodes, O.as_array(othr), L, bufs[0].value, least + 64, bufs[0].value, least + 64)
        assert np.array_equal(down(bufs[0]), out_of_place)                      # in place: the same bytes, the fill kept

        def refused(words, **change):
            args = dict(nodes=nodes, othr=O.as_array(othr), n_sites=L, in_ptr=bufs[0].value, in_stride=least + 64,
                        out_ptr=bufs[1].value, out_stride=least + 64)
            with pytest.raises(abn.AbnError) as e:
                S.observe_dev(gpu_ctx, SEED, **{**args, **change})
            assert e.value.status == 1 and words in str(e.value), str(e.value)

        refused("16-byte aligned", in_ptr=bufs[0].value + 8, in_stride=least)
        refused("16-byte aligned", out_ptr=bufs[1].value + 8, out_stride=least)
        refused("overlap other than in place", out_ptr=bufs[0].value + least + 64)     # one row further: a partial overlap
        refused("overlap other than in place", out_ptr=bufs[0].value, out_stride=least)
        bad = O.as_array(othr).copy()
        bad[2] = (9, 3, 10)
        refused("othr[2] decreases", othr=bad)
        refused("row_stride", in_stride=least - 64)
        refused("row_stride", out_stride=least + 32)
        refused("null pointer", out_ptr=0)
        assert np.array_equal(down(bufs[0]), out_of_place) and np.array_equal(down(bufs[1]), out_of_place)   # nothing launched
    finally:
        for ptr in bufs:
            hip.hipFree(ptr)


def test_past_the_first_grid_stride_trip(gpu_ctx):
    """two rows; the first lanes of the grid's x extent make a second trip"""
    blocks, threads = S.launch_grid(gpu_ctx, 1 << 34)
    L = 16 * threads * blocks + 16 * 300 + 5
    assert S.launch_grid(gpu_ctx, L) == (blocks, threads)
    rng = np.random.default_rng(34)
    packed, othr = M.pack(truth(rng, 2, L)), O.random_othr(rng)
    got = S.observe(gpu_ctx, SEED, packed, [7, 1], O.as_array(othr), L)
    assert np.array_equal(got, O.observe(SEED, packed, [7, 1], othr, L))


def test_thresholds_at_the_ends_and_equal(gpu_ctx):
    rng = np.random.default_rng(35)
    L, nodes = 1025, [3, 0]
    packed = M.pack(truth(rng, 2, L))
    base = O.random_othr(rng)
    cases = [[[0, 0, 0]] * 3, [[M.MAX64] * 3] * 3, [[0, 0, M.MAX64]] * 3, [[0, M.MAX64, M.MAX64]] * 3]
    for s in range(3):
        for i in range(3):
            for value in (0, M.MAX64):                                         # 0 and 2^64 - 1 in every position
                othr = [list(row) for row in base]
                othr[s][i] = value
                othr[s] = ([value] * (i + 1) + othr[s][i + 1:]) if value == 0 else (othr[s][:i] + [value] * (3 - i))
                cases.append(othr)
        for i in range(2):                                                     # equal pairs
            othr = [list(row) for row in base]
            othr[s][i + 1] = othr[s][i]
            cases.append(othr)
    for othr in cases:
        assert np.array_equal(S.observe(gpu_ctx, SEED, packed, nodes, O.as_array(othr), L), O.observe(SEED, packed, nodes, othr, L)), othr
    all_kept = O.unpack(S.observe(gpu_ctx, SEED, packed, nodes, O.as_array(cases[1]), L), L)
    assert (all_kept[O.unpack(packed, L) < 3] == 0).all()                       # w >= 2^64 - 1 never (the draws here)
    all_gone = O.unpack(S.observe(gpu_ctx, SEED, packed, nodes, O.as_array(cases[0]), L), L)
    assert (all_gone == 3).all()                                               # w >= 0 three times


def test_planted_ties(gpu_ctx):
    """A threshold whose high word is the draw's H word at site 37 and whose low word is Lw - 1, Lw, Lw + 1, for each of the
    three thresholds under each of the three true states: the lazy path draws the low words for that quad"""
    L, at, node = 64, 37, 6
    hi, lo = O.obs_draw_words(SEED, node, L)
    assert 0 < int(lo[at]) < 0xFFFFFFFF
    for which in range(3):
        for delta in (-1, 0, 1):
            for state in range(3):
                t = (int(hi[at]) << 32) | (int(lo[at]) + delta)
                othr = [[0, 0, M.MAX64] for _ in range(3)]
                othr[state] = [[t, M.MAX64, M.MAX64], [0, t, M.MAX64], [0, 0, t]][which]
                reached = which + (1 if delta <= 0 else 0)                     # the thresholds below `which` are 0: reached
                packed = M.pack(np.full((1, L), state, dtype=np.uint8))
                got = S.observe(gpu_ctx, SEED, packed, [node], O.as_array(othr), L)
                assert O.unpack(got, L)[0, at] == reached, (which, delta, state)
                assert np.array_equal(got, O.observe(SEED, packed, [node], othr, L)), (which, delta, state)


def test_properties_of_the_law(gpu_ctx):
    rng = np.random.default_rng(36)
    L, nodes = 4097, [2, 9, 4, 0]
    fields, othr = truth(rng, 4, L), O.as_array(O.obs_thresholds(*O.noise(0.05, 0.1)))
    whole = O.unpack(S.observe(gpu_ctx, SEED, M.pack(fields), nodes, othr, L), L)
    for shorter in (1, 16, 1000, 4096):                                        # the first L' sites of a run of L are the run of L'
        got = S.observe(gpu_ctx, SEED, M.pack(fields[:, :shorter]), nodes, othr, shorter)
        assert np.array_equal(O.unpack(got, shorter), whole[:, :shorter])
    for pick in ([1, 3], [3], [0, 1, 2]):                                      # a row's observation: its node's, whichever rows are there
        got = S.observe(gpu_ctx, SEED, M.pack(fields[pick]), [nodes[r] for r in pick], othr, L)
        assert np.array_equal(O.unpack(got, L), whole[pick])
    swapped = O.unpack(S.observe(gpu_ctx, SEED, M.pack(fields[[0, 0]]), [nodes[0], nodes[1]], othr, L), L)
    assert np.array_equal(swapped[0], whole[0]) and not np.array_equal(swapped[1], whole[0])      # another node: other draws
    assert not np.array_equal(O.unpack(S.observe(gpu_ctx, SEED + 1, M.pack(fields), nodes, othr, L), L), whole)


# ------------------------------------------------------------------------------------------------ the census
def census_windows(L):
    cuts = [c for c in CUTS if c <= L] + [L]
    begin, end = [], []
    for b in cuts:
        for e in cuts:
            if b <= e:
                begin.append(b), end.append(e)
    for b, e in ((100, 100), (40_000, 41_000), (1000, 40_000), (30_000, 50_000), (300, 68_000)):
        begin.append(b), end.append(e)       # empty, wholly filtered, two overlapping, three chunks and more
    return begin, end


@pytest.fixture(scope="module")
def census_case():
    rng = np.random.default_rng(8)
    L = 70_001
    fields = rng.integers(0, 4, size=(9, L), dtype=np.uint8)
    fields[:, 40_000:41_000] = 3
    begin, end = census_windows(L)
    return L, fields, begin, end, O.census(fields, begin, end)


@pytest.mark.parametrize("n", (9, 1, 2))
def test_census_equals_numpy_and_the_host_form(gpu_ctx, census_case, n):
    L, fields, begin, end, want = census_case
    packed = M.pack(fields[:n], stride=M.row_stride(L) + 128, fill=0x5A)
    got = Cn.census_windows(gpu_ctx, packed, L, begin, end)
    assert got.shape == (len(begin), n, 3) and np.array_equal(got, want[:, :n])
    assert np.array_equal(got, Cn.census_windows_host(packed, L, begin, end))
    assert not got[begin.index(100)].any() and not got[begin.index(40_000)].any()
    assert Cn.census_windows(gpu_ctx, packed, L, [], []).shape == (0, n, 3)


def test_census_device_entry(abn, gpu_ctx, hip, census_case):
    L, fields, begin, end, want = census_case
    packed = M.pack(fields, stride=M.row_stride(L) + 128, fill=0x5A)
    bufs = [C.c_void_p(), C.c_void_p()]
    assert hip.hipMalloc(C.byref(bufs[0]), packed.nbytes) == 0 and hip.hipMalloc(C.byref(bufs[1]), want.nbytes) == 0
    try:
        assert hip.hipMemcpy(bufs[0], packed.ctypes.data, packed.nbytes, 1) == 0
        assert hip.hipMemset(bufs[1], 0x5A, want.nbytes) == 0
        ms = Cn.census_windows_dev(gpu_ctx, bufs[0].value, 9, L, packed.shape[1], begin, end, bufs[1].value)
        assert ms > 0
        got = np.zeros_like(want)
        assert hip.hipMemcpy(got.ctypes.data, bufs[1], got.nbytes, 2) == 0
        assert np.array_equal(got, want)
        for words, change in (("16-byte aligned", dict(packed_ptr=bufs[0].value + 8)), ("row_stride_bytes", dict(row_stride=packed.shape[1] - 192)),
                              ("window 1 is not a column range", dict(begin=[0, 5], end=[10, L + 1])), ("null/size", dict(counts_ptr=0))):
            args = dict(packed_ptr=bufs[0].value, n_samples=9, n_sites=L, row_stride=packed.shape[1], begin=begin, end=end,
                        counts_ptr=bufs[1].value)
            with pytest.raises(abn.AbnError) as e:
                Cn.census_windows_dev(gpu_ctx, **{**args, **change})
            assert e.value.status == 1 and words in str(e.value), str(e.value)
    finally:
        for ptr in bufs:
            hip.hipFree(ptr)


# ------------------------------------------------------------------------------------------------ the study
@pytest.fixture(scope="module")
def study_case():
    parent, generation = M.TREE8
    thr = S.thresholds(parent, generation, *RATES).tolist()
    clean = O.study(STUDY_SEED, parent, generation, [1] * 8, thr, None, STUDY_L, STUDY_R)
    othr = O.obs_thresholds(*O.noise(0.02, 0.1))
    noisy = O.study(STUDY_SEED, parent, generation, [1] * 8, thr, othr, STUDY_L, STUDY_R)
    return parent, generation, thr, clean, noisy


def test_study_equals_the_model(gpu_ctx, study_case):
    parent, generation, thr, clean, noisy = study_case
    for want, noise in ((clean, {}), (noisy, dict(zip(("miscall", "dropout"), O.noise(0.02, 0.1))))):
        times, D, p0uu, census, ms = S.study(gpu_ctx, STUDY_SEED, parent, generation, [1] * 8, *RATES, STUDY_L, STUDY_R,
                                             with_ms=True, **noise)
        assert times.shape == (28, 3) and np.array_equal(times, want[0])
        assert D.shape == (STUDY_R, 28) and np.array_equal(D, want[1])
        assert np.array_equal(p0uu, want[2]) and np.array_equal(census, want[3])
        assert ms[0] > 0 and ms[2] > 0 and ms[3] > 0 and (ms[1] > 0) == bool(noise)
    assert not np.array_equal(clean[1], noisy[1])


def test_replicates_are_the_columns_of_one_simulation(abn, gpu_ctx, study_case):
    parent, generation, thr, clean, _ = study_case
    whole = S.codes(gpu_ctx, STUDY_SEED, parent, M.as_array(thr), [1] * 8, STUDY_R * STUDY_L)
    fields = abn.unpack_codes(whole, STUDY_R * STUDY_L)
    assert np.array_equal(fields, clean[5])
    for r in range(STUDY_R):
        assert np.array_equal(fields[:, r * STUDY_L:(r + 1) * STUDY_L], clean[5][:, r * STUDY_L:(r + 1) * STUDY_L])
        assert np.array_equal(O.census(fields[:, r * STUDY_L:(r + 1) * STUDY_L], [0], [STUDY_L])[0], clean[3][r])


def test_one_replicate_without_noise_is_the_pedigree(gpu_ctx):
    parent, generation = M.TREE8
    emit = [1, 0, 1, 1, 0, 1, 1, 1]
    rows, p0uu = S.pedigree(gpu_ctx, 7, parent, generation, emit, *RATES, STUDY_L)
    times, D, p, census = S.study(gpu_ctx, 7, parent, generation, emit, *RATES, STUDY_L, 1)
    assert np.array_equal(times, rows[:, :3]) and np.array_equal(D[0], rows[:, 3]) and p[0] == p0uu
    assert (census.sum(axis=2) == STUDY_L).all()


def test_statistics_of_the_study(gpu_ctx, oracle, study_case):
    """Without noise every D[r] lies within 6 sqrt(dt / L) of the model's dt1t2 (a site's |s_i - s_j| / 2 lies in {0, 1/2, 1}:
    its variance is at most its mean).  With E = 0 and F = 0.1 a site is kept by both samples of a pair with q = 0.9^2 =
    0.81, sites independently: `both` is binomial(L, q), within 6 sqrt(L q (1 - q)) of L q."""
    parent, generation, thr, clean, _ = study_case
    alpha, beta, p_uu0, w = RATES
    rows = np.concatenate([clean[0], clean[1][0][:, None]], axis=1)
    dt, _ = oracle.divergence(rows, 1.0 - p_uu0, p_uu0, alpha, beta, w)
    times, D, _, _ = S.study(gpu_ctx, STUDY_SEED, parent, generation, [1] * 8, *RATES, STUDY_L, STUDY_R)
    for r in range(STUDY_R):
        for k in range(28):
            assert abs(D[r, k] - dt[k]) <= 6.0 * np.sqrt(dt[k] / STUDY_L), (r, k, D[r, k], dt[k])
    L, R, q = STUDY_L, STUDY_R, 0.81
    othr = S.obs_thresholds(*O.noise(0.0, 0.1))
    packed = S.codes(gpu_ctx, STUDY_SEED, parent, M.as_array(thr), [1] * 8, R * L)
    seen = S.observe(gpu_ctx, STUDY_SEED, packed, list(range(8)), othr, R * L)
    _, both, _ = gpu_ctx.pairwise_divergence_windows_packed(seen, R * L, [r * L for r in range(R)], [(r + 1) * L for r in range(R)])
    assert both.shape == (R, 28)
    assert (np.abs(both.astype(np.float64) - L * q) <= 6.0 * np.sqrt(L * q * (1.0 - q))).all(), both
    _, _, _, census = S.study(gpu_ctx, STUDY_SEED, parent, generation, [1] * 8, *RATES, L, R, dropout=[0.1] * 3)
    assert np.array_equal(census, Cn.census_windows(gpu_ctx, seen, R * L, [r * L for r in range(R)], [(r + 1) * L for r in range(R)]))


def test_refusals_of_the_study(abn, gpu_ctx):
    parent, generation = M.TREE8

    def refused(words, emit=(1,) * 8, L=100, R=2):
        with pytest.raises(abn.AbnError) as e:
            S.study(gpu_ctx, 1, parent, generation, list(emit), *RATES, L, R)
        assert e.value.status == 1 and words in str(e.value), str(e.value)

    refused("above 2^34", L=1 << 20, R=(1 << 14) + 1)
    refused("fewer than one replicate", R=0)
    refused("no site", L=0)
    refused("fewer than two emitted nodes", emit=(0, 0, 0, 0, 0, 0, 0, 1))


def test_plan_of_the_replicates_is_the_command_line_tools_table(abn, gpu_ctx, tmp_path):
    """times / D / p0uu of the study as the windows of one Plan (window id = the replicate, no bootstraps), the fitted models
    through bootstrap_rows: the rows of the simulation_raw.npy `alphabeta --simulate .. --sim-replicates 5` writes for the
    same seed and starts"""
    from test_sim_cli_gpu import LISTS, alphabeta, golden_tree

    parent, generation, emit = golden_tree()
    seed, L, R, starts = 77, STUDY_L, 5, 6
    r = alphabeta("--simulate", "2e-3,5e-3", "--sim-sites", L, "--seed", seed, "-i", 20, "--sim-replicates", R, "--sim-starts", starts,
                  "--sim-miscall", 0.02, "--sim-dropout", 0.1, *LISTS, "-o", tmp_path)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    written = np.load(tmp_path / "simulation_raw.npy")
    assert written.shape == (R, 7) and np.isfinite(written).all()
    miscall, dropout = O.noise(0.02, 0.1)
    times, D, p0uu, _ = S.study(gpu_ctx, seed, parent, generation, emit, 2e-3, 5e-3, 0.75, 0.5, L, R, miscall=miscall, dropout=dropout)
    options = abn.default_options()
    options.seed = seed
    plan = abn.Plan(gpu_ctx, times, R, starts, 0, options=options)
    plan.set_window_ids(np.arange(R))
    plan.set_windows(D, p0uu)
    plan.run()
    models = plan.download(want_info=False)["models"]
    plan.close()
    assert np.array_equal(gpu_ctx.bootstrap_rows(models), written)
