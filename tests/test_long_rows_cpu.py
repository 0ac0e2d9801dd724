"""The periodic-row model of tests/_long_rows_model.py — the reference of tests/test_long_rows_gpu.py at rows of 2^26 to 2^34
sites — against brute force at rows short enough to build: its tables, folds and census against tests/_transitions_model.py
and tests/_sim_obs_model.py on the materialised view, and against the serial host forms; and the slice forms of the
simulation and observation models against slices of the whole ones.  Exact integers, floats bit for bit."""
import ctypes as C

import numpy as np
import pytest

import _long_rows_model as LR
import _sim_model as SM
import _sim_obs_model as OM
import _transitions_model as TM

LENGTHS = [49_263, 49_264, 49_265, 200_003]     # either side of the packed site period 4 P = 49 264, and several periods
N = 3


def windows_of(L):
    """the edge windows of _transitions_model (every residue of begin and end mod 256 and mod 16 they hold) as they are,
    stretched to the row's end region — across the period's end — and moved there; the row's ends; whole periods"""
    b, e = TM.edge_windows()
    shift = (L - TM.SITES) // 256 * 256
    assert shift > 0 and (e + shift).max() <= L
    begin = np.concatenate([b, b, b + shift, [0, L, L - 7, 0, 5, LR.P]])
    end = np.concatenate([e, e + shift, e + shift, [L, L, L, 0, min(L, 5 + 4 * LR.P), min(L, 5 * LR.P)]])
    return begin.astype(np.int64), end.astype(np.int64)


def test_windows_keep_the_residues_of_the_edge_list():
    b, e = TM.edge_windows()
    for L in LENGTHS:
        begin, end = windows_of(L)
        for m in (256, 16):
            assert {int(x) % m for x in begin} >= {int(x) % m for x in b}
            assert {int(x) % m for x in end} >= {int(x) % m for x in e}
        assert np.all(begin <= end) and end.max() == L and np.any((begin < 4 * LR.P) & (end > 4 * LR.P)) == (L > 4 * LR.P)


@pytest.fixture(scope="module")
def serial():
    from _build_many import hostlib

    fn = hostlib().abh_transitions_packed
    fn.restype = None
    fn.argtypes = [C.c_void_p, C.c_int, C.c_longlong, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]

    def run(packed, begin, end):
        packed = np.ascontiguousarray(packed, dtype=np.uint8)
        n, stride = packed.shape
        b, e = np.ascontiguousarray(begin, dtype=np.int64), np.ascontiguousarray(end, dtype=np.int64)
        out = np.full((len(b), n * (n - 1) // 2, 3, 3), 7, dtype=np.uint64)
        fn(packed.ctypes.data, n, stride, b.ctypes.data, e.ctypes.data, len(b), out.ctypes.data)
        return out

    return run


def test_the_period():
    for kind in ("packed", "bytes"):
        per = LR.period(3, kind)
        assert per.shape == (LR.P,) and per.dtype == np.uint8 and np.array_equal(per, LR.period(3, kind))
        assert not np.array_equal(per, LR.period(4, kind))
    assert LR.P % 4 == 0 and LR.P % 8 != 0 and (4 * LR.P) % 256 != 0 and LR.P // 4 == 3079
    assert all(3079 % d for d in range(2, 56))                                           # a prime: P has no other factor
    f = LR.View(LR.period(3, "packed"), "packed", 1, 4 * LR.P).fields[0]
    share = np.bincount(f, minlength=4) / f.size
    assert np.all(np.abs(share - np.array([0.4275, 0.095, 0.4275, 0.05])) < 0.01)
    by = LR.period(3, "bytes")
    assert set(np.unique(by)) <= {0, 1, 2, 0x80, 0x81, 0x82} and 0.03 < (by >= 0x80).mean() < 0.07
    assert 0.07 < ((by & 3) == 1).mean() < 0.13


def test_the_views_unpacking_is_the_formats():
    """the model's own unpacking of a period against _sim_obs_model.unpack (rows of whole 64-byte steps: the period padded)"""
    per = LR.period(5, "packed")
    v = LR.View(per, "packed", 2, 4 * LR.P)
    for r in range(2):
        row = np.concatenate([np.roll(per, -v.phase(r)), np.zeros(64, dtype=np.uint8)])[: SM.row_stride(4 * LR.P)]
        assert np.array_equal(OM.unpack(row.reshape(1, -1), 4 * LR.P)[0], v.fields[r])


@pytest.mark.parametrize("slack", [0, 64])
@pytest.mark.parametrize("L", LENGTHS)
def test_packed_views_against_brute_force(abn, oracle, serial, L, slack):
    from alphabeta_rs_amd import census

    per = LR.period(L, "packed")
    view = LR.View(per, "packed", N, L, LR.packed_stride(L) + slack)
    assert view.least == abn.packed_row_stride(L) == SM.row_stride(L)
    assert len({view.phase(r) for r in range(N)}) == N
    packed = view.rows(view.materialise())
    fields = OM.unpack(packed, L)                                                        # 0..3
    padding = OM.unpack(packed[:, : view.least], 4 * view.least)[:, L:]
    assert np.all(padding == 3)                                                          # the tails the model supplies
    codes = np.where(fields == 3, 0x80, fields).astype(np.uint8)
    begin, end = windows_of(L)
    got = view.tables(begin, end)
    assert got.dtype == np.int64 and np.array_equal(got.astype(np.uint64), TM.windows_table(codes, begin, end))
    assert np.array_equal(got.astype(np.uint64), serial(packed, begin, end))
    both, diff = LR.folds(got)
    wb, wd = TM.folds(TM.windows_table(codes, begin, end))
    assert np.array_equal(both.astype(np.uint64), wb) and np.array_equal(diff.astype(np.uint64), wd)
    cen = view.census(begin, end)
    assert np.array_equal(cen.astype(np.uint64), OM.census(fields, begin, end))
    assert np.array_equal(cen.astype(np.uint64), census.census_windows_host(packed, L, begin, end))
    assert np.array_equal(cen.astype(np.uint64), census.census_windows_host(packed, L, begin, end, walk_chunk=512))
    # the whole padded row counts what [0, L) counts: the patched tail reads as filtered
    whole = view.tables([0], [L])
    assert np.array_equal(serial(packed[:, : view.least], [0], [4 * view.least]), whole.astype(np.uint64))
    # D of the whole rows: the oracle's bits
    wb, wd = LR.folds(whole[0])
    od, ob, ov = oracle.pairwise_divergence(fields & 3, np.where(fields == 3, 0.5, 1.0), 0.99)
    assert np.array_equal(od, wd.astype(np.uint64)) and np.array_equal(ob, wb.astype(np.uint64))
    assert np.array_equal(LR.dvalue(wd, wb), ov, equal_nan=True)
    assert np.isnan(LR.dvalue(np.zeros(1, dtype=np.int64), np.zeros(1, dtype=np.int64))[0])


@pytest.mark.parametrize("L", LENGTHS)
def test_byte_views_against_brute_force(oracle, L):
    per = LR.period(L + 1, "bytes")
    view = LR.View(per, "bytes", N, L)
    assert view.stride == L and len({view.phase(r) for r in range(N)}) == (N if L % LR.P else 1)   # 49 264 bytes: 4 periods
    codes = view.rows(view.materialise())
    assert codes.shape == (N, L) and view.end_of_buffer() == N * L
    begin, end = windows_of(L)
    begin, end = np.minimum(begin + np.arange(len(begin)) % 2, end), end              # odd begins among them
    got = view.tables(begin, end)
    want = TM.windows_table(codes, begin, end)
    assert np.array_equal(got.astype(np.uint64), want)
    both, diff = LR.folds(got)
    wb, wd = TM.folds(want)
    assert np.array_equal(both.astype(np.uint64), wb) and np.array_equal(diff.astype(np.uint64), wd)
    od, ob, ov = oracle.pairwise_divergence(codes & 3, np.where(codes & 0x80, 0.5, 1.0), 0.99)
    wb, wd = LR.folds(view.tables([0], [L])[0])
    assert np.array_equal(od, wd.astype(np.uint64)) and np.array_equal(ob, wb.astype(np.uint64))
    assert np.array_equal(LR.dvalue(wd, wb), ov, equal_nan=True)


def test_more_samples_than_one_block():
    """n = 17: the prefix counts by planes against the bincount form, pair by pair"""
    L = 60_001
    view = LR.View(LR.period(17, "packed"), "packed", 17, L)
    fields = OM.unpack(view.rows(view.materialise()), L)
    codes = np.where(fields == 3, 0x80, fields).astype(np.uint8)
    begin, end = np.array([0, 49_000, 123]), np.array([L, 49_500, 59_999])
    assert np.array_equal(view.tables(begin, end).astype(np.uint64), TM.windows_table(codes, begin, end))
    assert np.array_equal(view.census(begin, end).astype(np.uint64), OM.census(fields, begin, end))


def test_the_chunk_rule():
    assert LR.chunk_of(0, 2048 * 32768, 32768, 256, 2048) == (32768, False, 2048)
    assert LR.chunk_of(0, 2048 * 32768 + 1, 32768, 256, 2048) == (32768 + 256, True, 2033)
    assert LR.chunk_of(261, 256 + 2048 * 32768, 32768, 256, 2048) == (32768, False, 2048)
    assert LR.chunk_of(1, 1 + 8192 * 8192, 8192, 1, 8192) == (8192, False, 8192)
    assert LR.chunk_of(1, 2 + 8192 * 8192, 8192, 1, 8192) == (8192 + 128, True, 8066)


# ---------------------------------------------------------------- the slice forms of the simulation and observation models
SEED = 0x9E3779B97F4A7C15
FIRSTS = [0, 16, 256, 1024, 4080, 4096]


def test_simulation_slices_are_slices_of_the_whole():
    L = 4097
    name, parent, generation, emit = SM.TREES[4]
    thr = SM.random_thresholds(np.random.default_rng(8), len(parent))
    whole = SM.states(SEED, parent, thr, L)
    for first in FIRSTS:
        for count in (1, 15, 16, 17, 257, L - first):
            count = min(count, L - first)
            assert np.array_equal(SM.states(SEED, parent, thr, count, first), whole[:, first: first + count]), (first, count)
            hi, lo = SM.draw_words(SEED, 3, count, first)
            whi, wlo = SM.draw_words(SEED, 3, L)
            assert np.array_equal(hi, whi[first: first + count]) and np.array_equal(lo, wlo[first: first + count])
    packed = SM.model(SEED, parent, thr, emit, L, fill=0x5A, stride=SM.row_stride(L) + 64)
    for first in (0, 256, 1024, 4096):                                     # whole super-steps: the padding is the row's own
        part = SM.model(SEED, parent, thr, emit, L - first, first=first)
        assert np.array_equal(part, packed[:, first // 4: SM.row_stride(L)])
    assert np.array_equal(SM.model(SEED, parent, thr, emit, 512, first=1024), packed[:, 256: 384])


def test_observation_slices_are_slices_of_the_whole():
    L = 4097
    rng = np.random.default_rng(9)
    nodes = [4, 0, 7]
    fields = rng.choice(4, size=(3, L), p=LR.WEIGHTS).astype(np.uint8)
    othr = OM.random_othr(rng)
    whole = OM.observe_fields(SEED, fields, nodes, othr)
    assert np.any(whole != fields)
    for first in FIRSTS:
        for count in (1, 17, 257, L - first):
            count = min(count, L - first)
            got = OM.observe_fields(SEED, fields[:, first: first + count], nodes, othr, first)
            assert np.array_equal(got, whole[:, first: first + count]), (first, count)
    packed = SM.pack(fields)
    seen = OM.observe(SEED, packed, nodes, othr, L)
    for first in (256, 4096):
        part = OM.observe(SEED, packed[:, first // 4:], nodes, othr, L - first, first=first)
        assert np.array_equal(part, seen[:, first // 4:])
