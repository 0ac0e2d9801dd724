"""The block bootstrap on the device (abn_block_*, abn_tiles_block_bootstrap; alphabeta_rs_amd/csrc/abn_blocks.hpp) against
the model of tests/_blocks_model.py, bit for bit: the product on the matrix pipe over every edge of rows, blocks, pairs,
groups, counts and digits, the accumulator flush, the counts on both sides of the histogram threshold, the device-pointer
entry and its flags, and the handle entry on pools and on fixed tiles against per-block tables the handle itself gives."""
import ctypes as C

import numpy as np
import pytest

import _blocks_model as M
import _tile_pools_model as PM
from test_tiles_gpu import ALIGNS, FLT, N, L, handles, inputs  # noqa: F401

pytestmark = pytest.mark.gpu
K = M.constants()
SEED = 20260101


@pytest.mark.parametrize("case", M.product_cases(), ids=lambda c: c[0])
def test_product_equals_the_model(gpu_ctx, case):
    gb, ge, counts, both, diff, lsk, kept = M.product_inputs(case)
    got = gpu_ctx.block_resample(gb, ge, counts, both, diff, lsk, kept)
    M.assert_equal(got, M.resample(gb, ge, counts, both, diff, lsk, kept))


@pytest.mark.parametrize("largest", [0, 127, 128, (1 << 14) - 1, 1 << 14, (1 << 28) - 1, 1 << 28], ids=str)
def test_every_number_of_digits(gpu_ctx, largest):
    """tables whose largest value needs 1, 1, 2, 2, 3, 4 and 5 digits"""
    rng = np.random.default_rng(largest % 1000)
    gb, ge = np.array([1, 70], dtype=np.int64), np.array([66, 200], dtype=np.int64)
    counts = M.planted_counts(rng, 2, 3, 200)
    both, diff, lsk, kept = M.tables(rng, 200, 3, 2, [0, largest, largest // 2, min(largest, 127)])
    got = gpu_ctx.block_resample(gb, ge, counts, both, diff, lsk, kept)
    M.assert_equal(got, M.resample(gb, ge, counts, both, diff, lsk, kept))


def test_accumulator_flush(gpu_ctx):
    args = M.flush_inputs(K["kBlockFlush"])
    got = gpu_ctx.block_resample(*args)
    T = K["kBlockFlush"] + 65
    assert int(got["both"][0, 0, 0]) == 127 * ((1 << 35) - 1) * T > 1 << 58
    M.assert_equal(got, M.resample(*args))


def test_a_jackknife_is_a_row_of_ones_with_one_zero(gpu_ctx):
    rng = np.random.default_rng(11)
    T = 70
    both, diff, lsk, kept = M.tables(rng, T, 3, 2, M.VALUES[:5])
    counts = (1 - np.eye(T, dtype=np.uint8))[None]
    got = gpu_ctx.block_resample([0], [T], counts, both, diff, lsk, kept)
    total = both.astype(object).sum(axis=0)
    assert [[int(v) for v in row] for row in got["both"][0]] == [[int(total[p] - both[t, p]) for p in range(3)] for t in range(T)]
    M.assert_equal(got, M.resample([0], [T], counts, both, diff, lsk, kept))


def test_product_refusals(abn, gpu_ctx):
    gb, ge, counts, both, diff, lsk, kept = M.product_inputs(M.product_cases()[4])
    over, big = counts.copy(), both.copy()
    over[0, 0, 3], big[1, 0] = 128, 1 << 35
    for args, words in (((gb, ge, over, both, diff, lsk, kept), "above 127"), ((gb, ge, counts, big, diff, lsk, kept), "2^35"),
                        ((gb, ge, counts, both, big, lsk, kept), "2^35")):
        with pytest.raises(abn.AbnError) as e:
            gpu_ctx.block_resample(*args)
        assert e.value.status == M.INVALID and words in str(e.value)


@pytest.fixture(scope="module")
def hip():
    lib = C.CDLL("libamdhip64.so")
    lib.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    lib.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    lib.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
    lib.hipFree.argtypes = [C.c_void_p]
    return lib


def test_device_resident_entry_and_its_flags(abn, gpu_ctx, hip):
    """tables, counts and results stay in HBM (buffers from the HIP runtime the product library already holds); a count of
    128 and a value of 2^35 the host never sees are found by the kernels"""
    case = ("dev", [5, 70, 77], [6, 70, 227], 17, 300, 45, 4)
    gb, ge, counts, both, diff, lsk, kept = M.product_inputs(case)
    want = M.resample(gb, ge, counts, both, diff, lsk, kept)
    over, big = counts.copy(), diff.copy()
    over[2, 16, 226], big[299 - 80, 44] = 128, 1 << 35
    ins = [counts, both, diff, lsk, kept, over, big]
    outs = [want[k] for k in ("both", "diff", "dvalue", "level", "kept")]
    bufs = [C.c_void_p() for _ in ins + outs]
    for ptr, a in zip(bufs, ins + outs):
        assert hip.hipMalloc(C.byref(ptr), a.nbytes) == 0
    try:
        for ptr, a in zip(bufs, ins):
            assert hip.hipMemcpy(ptr, a.ctypes.data, a.nbytes, 1) == 0
        d = [b.value for b in bufs]
        for skip in (None, 0, 2, 3):                                             # all outputs; then some of them not wanted
            for ptr, a in zip(bufs[7:], outs):
                assert hip.hipMemset(ptr, 7, a.nbytes) == 0
            o = [0 if k == skip else d[7 + k] for k in range(5)]
            ms = gpu_ctx.block_resample_dev(gb, ge, 17, d[0], 300, 45, 4, d[1], d[2], d[3], d[4], *o)
            assert ms.shape == (5,) and ms[0] == 0 and np.all(ms[1:] >= 0) and ms[2] > 0
            for k, w in enumerate(outs):
                host = np.zeros_like(w)
                assert hip.hipMemcpy(host.ctypes.data, bufs[7 + k], w.nbytes, 2) == 0
                if k == skip:
                    assert np.all(host.view(np.uint8) == 7)                      # untouched
                else:
                    assert host.tobytes() == w.tobytes(), k
        for counts_ptr, diff_ptr, words in ((d[5], d[2], "above 127"), (d[0], d[6], "2^35")):
            with pytest.raises(abn.AbnError) as e:
                gpu_ctx.block_resample_dev(gb, ge, 17, counts_ptr, 300, 45, 4, d[1], diff_ptr, d[3], d[4], *d[7:])
            assert e.value.status == M.INVALID and words in str(e.value)
    finally:
        for ptr in bufs:
            hip.hipFree(ptr)


@pytest.fixture(scope="module")
def count_groups():
    sizes = M.count_group_sizes(K["kBlockHist"])
    gb = np.concatenate([[2], 2 + np.cumsum(sizes)[:-1] + np.arange(1, len(sizes))]).astype(np.int64)   # a gap between groups
    gid = np.array([7, 0, 3, 4095, 11, 12, 13, 2 ** 32 - 1], dtype=np.uint32)
    return sizes, gid, gb, gb + np.array(sizes), int(gb[-1] + sizes[-1]) + 3


def test_counts_equal_the_model(abn, gpu_ctx, oracle, count_groups):
    sizes, gid, gb, ge, T = count_groups
    got = gpu_ctx.block_counts(SEED, gid, gb, ge, 2, T)
    want = M.counts(oracle, SEED, gid, gb, ge, 2, T)
    assert got.dtype == np.uint8 and got.shape == want.shape and got.tobytes() == want.tobytes()
    assert got.tobytes() == abn.block_counts_host(SEED, gid, gb, ge, 2, T).tobytes()
    for g, size in enumerate(sizes):
        assert got[g].sum(axis=1, dtype=np.int64).tolist() == [size] * 3         # every row makes exactly T_g draws
        assert got[g, 2, gb[g]:ge[g]].tolist() == [1] * size                     # the identity row
        assert got[g, :, :gb[g]].sum() == 0 == got[g, :, ge[g]:].sum()
    assert gpu_ctx.block_counts(SEED, gid, gb, ge, 2, T).tobytes() == got.tobytes()   # two calls, the same bytes


def test_counts_rows_depend_on_neither_R_nor_G(abn, gpu_ctx, count_groups):
    sizes, gid, gb, ge, T = count_groups
    few = gpu_ctx.block_counts(SEED, gid, gb, ge, 2, T)
    more = gpu_ctx.block_counts(SEED, gid, gb, ge, 19, T)
    assert more[:, :2].tobytes() == few[:, :2].tobytes() and more[:, 19].tobytes() == few[:, 2].tobytes()
    part = gpu_ctx.block_counts(SEED, gid[4:7], gb[4:7], ge[4:7], 2, T)
    assert part.tobytes() == few[4:7].tobytes()
    assert more.tobytes() == abn.block_counts_host(SEED, gid, gb, ge, 19, T).tobytes()
    assert gpu_ctx.block_counts(SEED + 1, gid, gb, ge, 2, T)[:, :2].tobytes() != few[:, :2].tobytes()
    for r in range(19):
        assert more[:, r].sum(dtype=np.int64) == sum(sizes)


def test_counts_refusals(abn, gpu_ctx):
    for args, words in (((1, [0], [0], [0], K["kBlockReplicatesMax"] + 1, 0), "replicates"), ((1, [0], [0], [0], -1, 0), "negative"),
                        ((1, [0], [2], [1], 1, 4), "unordered"), ((1, [0], [0], [5], 1, 4), "unordered"),
                        ((1, [0, 1], [0, 2], [3, 4], 1, 4), "overlaps"),
                        ((1, np.zeros(4097), np.zeros(4097), np.zeros(4097), 1, 0), "4096 groups")):
        with pytest.raises(abn.AbnError) as e:
            gpu_ctx.block_counts(*args)
        assert e.value.status == M.INVALID and words in str(e.value), args


# ---------------------------------------------------------------- the handle
R = 3


def per_block_tables(abn, gpu_ctx, sites, align, intervals):
    """the tables of a block list as a second handle's set_intervals gives them: both, diff (T, pairs), lsk, kept (n, T)"""
    second = abn.Tiles.from_parsed(gpu_ctx, sites, posterior_max_filter=FLT, align=align)
    try:
        second.set_intervals(*intervals)
        diff, both, _ = second.pairwise()
        _, lsk, kept = second.stats()
        return both, diff, lsk, kept
    finally:
        second.close()


@pytest.fixture(scope="module")
def pool_counts(oracle, inputs):
    """the model's counts of the pools' segments: the segment list is the same under every alignment"""
    made = {}

    def of(first):
        key = tuple(first)
        if key not in made:
            gb, ge = np.array(first[:-1], dtype=np.int64), np.array(first[1:], dtype=np.int64)
            made[key] = (gb, ge, M.counts(oracle, SEED, np.arange(len(gb)), gb, ge, R, int(first[-1])))
        return made[key]

    return of


@pytest.mark.parametrize("align", ALIGNS)
def test_pooled_handle(abn, gpu_ctx, inputs, handles, pool_counts, align):
    rows, values, keeps = inputs
    h = handles[align]
    tiles = h["tiles"]
    (ic, ilo, ihi, ip), names, _ = PM.pool_list(rows)
    tiles.set_pools(ic, ilo, ihi, ip, len(names))
    out = tiles.block_bootstrap(SEED, R)
    # the identity rows are the pooled handle's own scan and folds
    diff, both, dval = tiles.pairwise()
    _, lsk, kept = tiles.stats()
    assert out["both"][:, R].tobytes() == both.tobytes() and out["diff"][:, R].tobytes() == diff.tobytes()
    assert out["dvalue"][:, R].tobytes() == dval.tobytes() and out["kept"][:, R].tobytes() == np.ascontiguousarray(kept.T).tobytes()
    # every row is the model's, fed with the per-segment tables set_intervals gives
    seg = tiles.pool_segments()
    first = np.searchsorted(seg[0], np.arange(len(names) + 1)).tolist()
    gb, ge, counts = pool_counts(first)
    assert [g.tolist() for g in tiles.block_groups()] == [gb.tolist(), ge.tolist()]
    tables = per_block_tables(abn, gpu_ctx, h["sites"], align, (seg[1], seg[2], seg[3]))
    M.assert_equal(out, M.resample(gb, ge, counts, *tables))
    sizes = (ge - gb).tolist()
    assert 1 in sizes and max(sizes) > 4096 and any(b % 64 for b in gb.tolist())   # ("nothing": blocks without a column)
    assert not out["both"][names.index("nothing")].any() and np.isnan(out["dvalue"][names.index("nothing")]).all()
    assert (out["both"][:, :R] != out["both"][:, R:]).any()                      # the replicates differ from the observed data
    ms = tiles.block_ms()
    assert ms.shape == (5,) and np.all(ms > 0)
    again = tiles.block_bootstrap(SEED, R)
    M.assert_equal(again, out)
    more = tiles.block_bootstrap(SEED, R + 2)                                    # a row depends on neither R nor G
    assert more["both"][:, :R].tobytes() == out["both"][:, :R].tobytes() and more["level"][:, R + 2].tobytes() == out["level"][:, R].tobytes()


@pytest.mark.parametrize("align", ALIGNS)
def test_fixed_tiles_handle(abn, gpu_ctx, oracle, inputs, handles, align):
    h = handles[align]
    tiles = h["tiles"]
    tiles.set_fixed(1 << 24)                                                     # some 260 tiles, most of them empty
    T = tiles.info()["n_tiles"]
    assert T > 64
    out = tiles.block_bootstrap(SEED, R)
    diff, both, dval = tiles.pairwise()
    _, lsk, kept = tiles.stats()
    gb, ge = np.array([0], dtype=np.int64), np.array([T], dtype=np.int64)
    assert [g.tolist() for g in tiles.block_groups()] == [[0], [T]]
    counts = M.counts(oracle, SEED, [0], gb, ge, R, T)
    M.assert_equal(out, M.resample(gb, ge, counts, both, diff, lsk, kept))
    assert out["both"][0, R].tobytes() == both.astype(object).sum(axis=0).astype(np.uint64).tobytes()
    tiles.set_fixed(1 << 24, 1 << 25)                                              # step >= size: gaps, no overlap
    assert tiles.block_bootstrap(SEED, 1)["both"].shape == (1, 2, N * (N - 1) // 2)


def test_handle_refusals(abn, gpu_ctx, inputs, handles):
    rows, values, keeps = inputs
    tiles = abn.Tiles.from_parsed(gpu_ctx, handles["none"]["sites"], posterior_max_filter=FLT)
    try:
        with pytest.raises(abn.AbnError) as e:                                   # no tiles yet
            tiles.block_bootstrap(SEED, 1)
        assert e.value.status == M.INVALID
        (ic, ilo, ihi, ip), names, _ = PM.pool_list(rows)
        for setter, args in ((tiles.set_intervals, (ic[:9], ilo[:9], ihi[:9])), (tiles.set_fixed, (1 << 28, 1 << 27))):
            setter(*args)
            with pytest.raises(abn.AbnError) as e:
                tiles.block_bootstrap(SEED, 1)
            assert e.value.status == M.INVALID and "overlap" in str(e.value)
        tiles.set_fixed(1 << 28, 1 << 28)
        tiles.block_bootstrap(SEED, 1)
        lib = gpu_ctx._L
        assert lib.abn_tiles_block_bootstrap(tiles._h, SEED, K["kBlockReplicatesMax"] + 1, None, None, None, None, None) == M.INVALID
        assert b"replicates" in lib.abn_last_error(gpu_ctx._h)
        assert lib.abn_tiles_block_bootstrap(tiles._h, SEED, 2, None, None, None, None, None) == 0      # no output wanted
        assert lib.abn_tiles_block_ms(tiles._h, None) == M.INVALID and lib.abn_tiles_block_ms(None, None) == M.INVALID
        tiles.set_pools(ic, ilo, ihi, ip, len(names))
        tiles.set_intervals(ic[:9], ilo[:9], ihi[:9])                            # pools dropped: refused again
        with pytest.raises(abn.AbnError):
            tiles.block_bootstrap(SEED, 1)
    finally:
        tiles.close()
