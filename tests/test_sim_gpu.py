"""The simulated methylomes on the device (abn_sim_codes*, abn_sim_pedigree through alphabeta_rs_amd.simulate) against the
numpy model of tests/_sim_model.py, bit for bit: the sizes around the dword, the 64-byte step, a wavefront and a workgroup
and one past the launch's first grid-stride trip; chains, stars, unemitted internal nodes and founders, dt = 0; thresholds
at the ends of their range, equal pairs and planted ties of the high word; the law's properties; the device-resident entry
and its stride; the pedigree of the 8-node tree against the model's dt1t2."""
import ctypes as C

import numpy as np
import pytest

import _sim_model as M
from alphabeta_rs_amd import simulate as S

pytestmark = pytest.mark.gpu
SEED = 0x9E3779B97F4A7C15
RATES = (0.1, 0.2, 0.7, 0.3)     # fast rates: every state and every transition occurs within a few sites


@pytest.fixture(scope="module")
def hip():
    h = C.CDLL("libamdhip64.so")        # the HIP runtime the product library already holds
    h.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    h.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    h.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
    h.hipFree.argtypes = [C.c_void_p]
    return h


@pytest.mark.parametrize("tree", M.TREES, ids=[t[0] for t in M.TREES])
def test_device_entry_equals_the_model(gpu_ctx, tree):
    name, parent, generation, emit = tree
    thr = S.thresholds(parent, generation, *RATES)
    anything = M.random_thresholds(np.random.default_rng(len(parent)), len(parent))
    for L in M.SIZES:
        assert np.array_equal(S.codes(gpu_ctx, SEED, parent, thr, emit, L), M.model(SEED, parent, thr.tolist(), emit, L)), L
        assert np.array_equal(S.codes(gpu_ctx, SEED, parent, M.as_array(anything), emit, L), M.model(SEED, parent, anything, emit, L)), L
    assert np.array_equal(S.codes(gpu_ctx, SEED, parent, thr, emit, 4097), S.codes_host(SEED, parent, thr, emit, 4097))


def test_past_the_first_grid_stride_trip(gpu_ctx):
    """three nodes, the founder unemitted (a scratch row): the first lanes of the grid make a second trip"""
    blocks, threads = S.launch_grid(gpu_ctx, 1 << 34)                      # the cap of the grid
    assert threads == 256 and blocks >= 1 and S.launch_grid(gpu_ctx, 16 * threads * blocks) == (blocks, threads)
    L = 16 * threads * blocks + 16 * 300 + 5
    assert S.launch_grid(gpu_ctx, L) == (blocks, threads)
    parent, generation, emit = [-1, 0, 0], [1, 2, 4], [0, 1, 1]
    thr = S.thresholds(parent, generation, *RATES)
    got = S.codes(gpu_ctx, SEED, parent, thr, emit, L)
    want = M.model(SEED, parent, thr.tolist(), emit, L)
    assert got.shape == want.shape and np.array_equal(got, want)
    assert S.launch_grid(gpu_ctx, 0)[0] == 0 and S.launch_grid(gpu_ctx, 1)[0] == 1 and S.launch_grid(gpu_ctx, 16 * 256 + 1)[0] == 2


def test_thresholds_at_the_ends_and_equal(gpu_ctx):
    parent, emit, L = [-1, 0, 1, 0], [1, 1, 1, 1], 1025
    rng = np.random.default_rng(5)
    base = M.random_thresholds(rng, 4)
    cases = [[[[0, 0]] * 3] * 4, [[[M.MAX64, M.MAX64]] * 3] * 4, [[[0, M.MAX64]] * 3] * 4]
    for v in range(4):
        for s in range(3):
            for pair in ([0, None], [None, M.MAX64], [0, 0], [M.MAX64, M.MAX64], [0, M.MAX64]):   # 0 and 2^64 - 1 in every position
                thr = [[list(p) for p in node] for node in base]
                thr[v][s] = [thr[v][s][k] if pair[k] is None else pair[k] for k in range(2)]
                cases.append(thr)
    equal = [[[t[0], t[0]] for t in node] for node in base]                                        # t0 == t1: no state 1 from them
    cases.append(equal)
    for thr in cases:
        assert np.array_equal(S.codes(gpu_ctx, SEED, parent, M.as_array(thr), emit, L), M.model(SEED, parent, thr, emit, L))
    st = abn_states(S.codes(gpu_ctx, SEED, parent, M.as_array(equal), emit, L), L)
    assert not (st == 1).any() and (st == 0).any() and (st == 2).any()
    st = abn_states(S.codes(gpu_ctx, SEED, parent, M.as_array(cases[0]), emit, L), L)
    assert (st == 2).all()                                                                         # u >= 0 twice


def abn_states(packed, L):
    import alphabeta_rs_amd as abn

    return abn.unpack_codes(packed, L)


def test_planted_ties(gpu_ctx):
    """A threshold whose high word is a draw's H word and whose low word is Lw - 1, Lw, Lw + 1, for both thresholds under a
    parent state of 0, 1 and 2: the lazy path draws the low words for that quad and decides as the law does"""
    for which in (0, 1):
        for delta in (-1, 0, 1):
            for state in (0, 1, 2):
                thr, wanted = M.planted(SEED, which, delta, state)
                got = S.codes(gpu_ctx, SEED, [-1, 0], M.as_array(thr), [1, 1], 64)
                st = abn_states(got, 64)
                assert (st[0] == state).all() and st[1][37] == wanted, (which, delta, state)
                assert np.array_equal(got, M.model(SEED, [-1, 0], thr, [1, 1], 64)), (which, delta, state)


def test_properties_of_the_law(gpu_ctx):
    name, parent, generation, emit = M.TREES[3]
    thr = S.thresholds(parent, generation, *RATES)
    L = 4097
    whole = S.codes(gpu_ctx, SEED, parent, thr, emit, L)
    st = abn_states(whole, L)
    for shorter in (1, 16, 1000, 4096):                                    # the first L' sites of a run of L are the run of L'
        assert np.array_equal(abn_states(S.codes(gpu_ctx, SEED, parent, thr, emit, shorter), shorter), st[:, :shorter])
    more = parent + [4, 0, 8]                                              # appended nodes leave earlier rows unchanged
    thr_more = np.concatenate([thr, M.as_array(M.random_thresholds(np.random.default_rng(1), 3))])
    longer = S.codes(gpu_ctx, SEED, more, thr_more, emit + [1, 1, 1], L)
    assert np.array_equal(longer[:8], whole)
    for pick in ([1, 0, 0, 1, 0, 1, 1, 0], [0, 0, 0, 0, 0, 0, 0, 1], [0, 1, 1, 1, 1, 1, 1, 1]):   # emit only selects rows
        assert np.array_equal(S.codes(gpu_ctx, SEED, parent, thr, pick, L), whole[np.flatnonzero(pick)])
    assert not np.array_equal(S.codes(gpu_ctx, SEED + 1, parent, thr, emit, L), whole)


def test_device_resident_entry_and_the_scan(abn, gpu_ctx, hip):
    name, parent, generation, emit = M.TREES[4]
    thr = S.thresholds(parent, generation, *RATES)
    L, n = 70_001, int(np.sum(emit))
    least = abn.packed_row_stride(L)
    want = S.codes(gpu_ctx, SEED, parent, thr, emit, L)
    assert np.array_equal(want, M.model(SEED, parent, thr.tolist(), emit, L))
    npairs = n * (n - 1) // 2
    bufs = [C.c_void_p() for _ in range(3)]
    stride = least + 128
    for ptr, size in zip(bufs, (n * stride, 8 * npairs, 8 * npairs)):
        assert hip.hipMalloc(C.byref(ptr), size) == 0
    try:
        for row_stride in (least, stride):
            assert hip.hipMemset(bufs[0], 0x5A, n * stride) == 0
            ms = S.codes_dev(gpu_ctx, SEED, parent, thr, emit, L, bufs[0].value, row_stride)
            assert ms > 0
            host = np.zeros((n, row_stride), dtype=np.uint8)
            assert hip.hipMemcpy(host.ctypes.data, bufs[0], host.nbytes, 2) == 0
            assert np.array_equal(host[:, :least], want)
            assert (host[:, least:] == 0x5A).all()                          # the bytes between the rows are not written
            ms = gpu_ctx.pairwise_divergence_packed_dev(bufs[0].value, n, L, row_stride, bufs[1].value, bufs[2].value, 0)
            assert ms > 0
            diff, both = np.zeros(npairs, dtype=np.uint64), np.zeros(npairs, dtype=np.uint64)
            assert hip.hipMemcpy(diff.ctypes.data, bufs[1], 8 * npairs, 2) == 0
            assert hip.hipMemcpy(both.ctypes.data, bufs[2], 8 * npairs, 2) == 0
            _, _, want_diff, want_both = M.pedigree(M.states(SEED, parent, thr.tolist(), L), parent, generation, emit)
            assert diff.tolist() == want_diff and both.tolist() == want_both
        with pytest.raises(abn.AbnError) as e:                              # refused before any launch
            S.codes_dev(gpu_ctx, SEED, parent, thr, emit, L, bufs[0].value + 8, stride)
        assert "16-byte aligned" in str(e.value)
        for words, change in (("row_stride", dict(row_stride=least - 64)), ("no emitted node", dict(emit=[0] * 8)),
                              ("parent[3] is not a node in front of it", dict(parent=[-1, 0, 0, 3, 1, 2, 2, 3])),
                              ("n_sites below 0", dict(n_sites=-1))):
            args = dict(parent=parent, thr=thr, emit=emit, n_sites=L, out_ptr=bufs[0].value, row_stride=stride)
            with pytest.raises(abn.AbnError) as e:
                S.codes_dev(gpu_ctx, SEED, **{**args, **change})
            assert e.value.status == 1 and words in str(e.value)
        with pytest.raises(abn.AbnError) as e:
            S.codes_dev(gpu_ctx, SEED, parent, thr, emit, L, 0, stride)
        assert "null pointer" in str(e.value)
    finally:
        for ptr in bufs:
            hip.hipFree(ptr)


def test_pedigree_of_the_eight_node_tree(abn, gpu_ctx, oracle):
    """rows in DMatrix::convert's order; every D within 6 sqrt(dt1t2 / L) of the model's dt1t2 (a site's |s_i - s_j| / 2 lies
    in {0, 1/2, 1}: its variance is at most its mean); D and p0uu equal the numpy model's to the bit"""
    parent, generation = M.TREE8
    alpha, beta, p_uu0, w, L = 2e-3, 5e-3, 0.7, 0.3, 400_000
    emit = [1] * 8
    rows, p0uu = S.pedigree(gpu_ctx, 20260101, parent, generation, emit, alpha, beta, p_uu0, w, L)
    thr = S.thresholds(parent, generation, alpha, beta, p_uu0, w)
    want_rows, want_p0uu, _, _ = M.pedigree(M.states(20260101, parent, thr.tolist(), L), parent, generation, emit)
    assert rows.shape == (28, 4) and np.array_equal(rows, want_rows)
    assert p0uu == want_p0uu
    pairs = [(i, j) for i in range(8) for j in range(i + 1, 8)]
    for r, (i, j) in enumerate(pairs):
        assert rows[r, 1] == generation[i] and rows[r, 2] == generation[j]
    assert rows[pairs.index((3, 4)), 0] == 3 and rows[pairs.index((3, 7)), 0] == 5 and rows[pairs.index((4, 5)), 0] == 2
    dt, _ = oracle.divergence(rows, 1.0 - p_uu0, p_uu0, alpha, beta, w)
    for r in range(28):
        assert abs(rows[r, 3] - dt[r]) <= 6.0 * np.sqrt(dt[r] / L), (rows[r], dt[r])
    some = [0, 1, 0, 1, 1, 0, 0, 1]                                        # unemitted nodes: the rows of the emitted pairs
    rows4, _ = S.pedigree(gpu_ctx, 20260101, parent, generation, some, alpha, beta, p_uu0, w, L)
    keep = [r for r, (i, j) in enumerate(pairs) if some[i] and some[j]]
    assert np.array_equal(rows4, rows[keep])
    model, _, _, _ = gpu_ctx.ab_neutral_run(rows, p0uu, p0uu, 1.0, 20)       # the result goes straight into the fit
    assert np.isfinite(model).all()
    with pytest.raises(abn.AbnError) as e:
        S.pedigree(gpu_ctx, 1, parent, generation, [0, 0, 0, 0, 0, 0, 0, 1], alpha, beta, p_uu0, w, L)
    assert "fewer than two emitted nodes" in str(e.value)
