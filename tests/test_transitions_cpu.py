"""The 3 x 3 state transitions of every sample pair (abn_pairwise_transitions*; the joint table behind DMatrix::from,
src/pedigree.rs:236-257) on the CPU: the serial host form of csrc/abn_pairwise_transitions.hpp, through the host shim,
against the numpy model of tests/_transitions_model.py and, folded to `both` and `diff`, against the oracle.  Exact
integers throughout."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

import _transitions_model as M

ROOT = Path(__file__).resolve().parent.parent
NEW_SYMBOLS = ["abn_pairwise_transitions_packed", "abn_pairwise_transitions_packed_dev",
               "abn_pairwise_transitions_windows_packed", "abn_pairwise_transitions_windows_packed_dev",
               "abn_codes_transitions", "abn_tiles_transitions"]


@pytest.fixture(scope="module")
def serial():
    from _build_many import hostlib

    L = hostlib()
    fn = L.abh_transitions_packed
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


@pytest.mark.parametrize("n", [1, 2, 3, 17])
@pytest.mark.parametrize("sites", [0, 1, 15, 16, 17, 255, 256, 257, 1000])
def test_serial_form_equals_the_model(abn, oracle, serial, n, sites):
    status, pmax, codes = M.random_codes(1000 * n + sites, n, sites)
    packed = abn.pack_codes(codes)
    assert packed.shape[1] % 64 == 0 and 4 * packed.shape[1] >= sites           # the row padding reads as filtered
    got = serial(packed, [0], [sites])[0]
    want = M.table(codes)
    assert got.shape == want.shape and np.array_equal(got, want)
    if n > 2 and sites:
        assert not got[1].any() and not got[n - 1 + 0].any()                   # pairs (0, 2) and (1, 2): sample 2 is all filtered
    # the whole padded row gives the same table: every field behind the last site is 3
    assert np.array_equal(serial(packed, [0], [4 * packed.shape[1]])[0], want)
    both, diff = M.folds(got)
    if n >= 2:
        od, ob, _ = oracle.pairwise_divergence(status, pmax, 0.99)
        assert np.array_equal(both, ob) and np.array_equal(diff, od)


@pytest.mark.parametrize("n", [2, 5])
def test_serial_windows_equal_the_model_on_the_edge_windows(abn, oracle, serial, n):
    status, pmax, codes = M.random_codes(n, n, M.SITES)
    begin, end = M.edge_windows()
    assert len(begin) >= 48 and (0, M.SITES) in set(zip(begin.tolist(), end.tolist()))
    got = serial(abn.pack_codes(codes), begin, end)
    assert np.array_equal(got, M.windows_table(codes, begin, end))
    both, diff = M.folds(got)
    for w, (b, e) in enumerate(zip(begin, end)):
        od, ob, _ = oracle.pairwise_divergence(status[:, b:e], pmax[:, b:e], 0.99)
        assert np.array_equal(both[w], ob) and np.array_equal(diff[w], od), (w, b, e)
    for w in np.flatnonzero(begin == end):
        assert not got[w].any()


def test_the_plane_form_of_the_model_equals_the_bincount_form():
    _, _, codes = M.random_codes(9, 19, 777)
    assert np.array_equal(M.table_by_planes(codes), M.table(codes))
    begin, end = np.array([0, 5, 300, 777]), np.array([777, 5, 641, 777])
    assert np.array_equal(M.windows_table_by_planes(codes, begin, end), M.windows_table(codes, begin, end))


def test_model_orientation_by_hand():
    """x is the state of the lower-numbered sample: U in a and M in b is entry [0, 2]"""
    a = np.array([0, 0, 0, 2, 1, 0x80, 0], dtype=np.uint8)
    b = np.array([2, 2, 1, 0, 1, 0, 0x82], dtype=np.uint8)
    t = M.pair_table(a, b)
    assert t.tolist() == [[0, 1, 2], [0, 1, 0], [1, 0, 0]]
    assert M.folds(t) == (5, 7)


def test_new_symbols_are_exported_and_documented(abn):
    L = abn.load_library()
    doc = (ROOT / "INTEGRATION.md").read_text()
    header = (ROOT / "include" / "abneutral.h").read_text()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name), name
        assert name in abn.EXPORTED_SYMBOLS and f"{name}(" in doc and f"{name}(" in header
