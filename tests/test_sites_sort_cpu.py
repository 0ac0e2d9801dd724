"""The sort of a methylome's records by genomic position in its serial forms (alphabeta_rs_amd/csrc/abn_sites_sort.hpp
through host_capi.cpp), against numpy.lexsort — stable, and never the code under test: the comparison sort, the digit
function, the walk of the radix passes workgroup by workgroup as the kernels make them, the pass-skip rule, and the native
program plain and under the address and undefined-behaviour sanitizers."""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import _sort_model as M

ROOT = Path(__file__).resolve().parent.parent
NEW_SYMBOLS = ["abn_sites_sort", "abn_sites_sort_order", "abn_sites_sort_info", "abn_sites_sort_keys", "abn_sites_sort_keys_dev"]


@pytest.fixture(scope="module")
def L():
    return M.hostlib()


def host_sort(L, k, walk=None):
    n = len(k[0])
    order, info = np.full(n, -1, dtype=np.int64), np.zeros(4, dtype=np.int64)
    ptrs = [a.ctypes.data for a in k]
    if walk is None:
        rc = L.abn_sites_sort_keys_host(n, *ptrs, order.ctypes.data, info.ctypes.data)
    else:
        rc = L.abh_sites_sort_walk(n, *ptrs, int(walk), order.ctypes.data, info.ctypes.data)
    assert rc == 0
    return order, info.tolist()


def test_serial_sort_equals_lexsort(L):
    assert M.tile(L) == 2048 and L.abh_sites_sort_passes() == M.PASSES
    for n in M.sizes(L):
        for name, k in M.patterns(n, seed=n):
            want, descents, equal = M.reference(k)
            order, info = host_sort(L, k)
            assert np.array_equal(order, want), (n, name)
            assert info == [n, descents, equal, M.passes_needed(k, descents)], (n, name)
            if name in ("all equal", "sorted"):
                assert np.array_equal(order, np.arange(n)) and info[1] == 0 and info[3] == 0
    for bit, k in M.bit_pairs():
        assert host_sort(L, k)[0].tolist() == [1, 0], bit


def test_digit_function_reads_every_key_bit_in_exactly_one_pass(L):
    seen = []
    for bit in range(M.KEY_BITS):
        digits = [L.abh_sites_sort_digit(*M.key_of_bit(bit), p) for p in range(M.PASSES)]
        assert digits == [(1 << (bit % 8)) if p == bit // 8 else 0 for p in range(M.PASSES)], bit
        seen.append(bit // 8)
    assert seen == sorted(seen)                                              # least significant first: strand, end, start, chromosome
    assert [L.abh_sites_sort_digit(257, 0xffffffff, 0xffffffff, 2, p) for p in range(M.PASSES)] == \
        [(M.key_int(257, 0xffffffff, 0xffffffff, 2) >> (8 * p)) & 0xff for p in range(M.PASSES)]
    assert len(M.bit_pairs()) == M.KEY_BITS


def test_walk_of_the_passes_equals_the_serial_sort_at_every_tile_edge(L):
    for n in M.sizes(L):
        for name, k in M.patterns(n, seed=1000 + n):
            want, descents, equal = M.reference(k)
            order, info = host_sort(L, k, walk=True)
            assert np.array_equal(order, want), (n, name)
            assert info == [n, descents, equal, M.passes_needed(k, descents)], (n, name)
    for bit, k in M.bit_pairs():
        order, info = host_sort(L, k, walk=True)
        assert order.tolist() == [1, 0] and info[1:] == [1, 0, 1], bit       # one descent: the one pass that holds the bit


def test_skipped_passes_change_nothing(L):
    t = M.tile(L)
    for n in (65, t + 1, 3 * t + 17):
        for name, k in M.patterns(n, seed=2000 + n):
            skipped, info = host_sort(L, k, walk=True)
            every, info_all = host_sort(L, k, walk=False)
            assert np.array_equal(skipped, every), (n, name)
            assert info_all[3] == (M.PASSES if info[1] else 0) and info[3] <= info_all[3]
            if name == "by strand":                                          # chromosomes below 256, short sites: constant digits
                assert 0 < info[3] < M.PASSES, info
            if name == "three values":
                assert info[3] == 3, info                                    # the bytes that hold bits 0-3, 34-35 and 66-67


def test_host_form_refusals(L):
    import alphabeta_rs_amd as abn

    for bad in ((258, 0, 0, 0), (-1, 0, 0, 0), (0, 0, 0, 3)):
        k = M.keys(*([0, v] for v in bad))
        order, info = np.zeros(2, dtype=np.int64), np.zeros(4, dtype=np.int64)
        assert L.abn_sites_sort_keys_host(2, *(a.ctypes.data for a in k), order.ctypes.data, info.ctypes.data) == 1
        with pytest.raises(abn.AbnError):
            abn.sort_sites_host(*k)
    order, info = abn.sort_sites_host([2, 1, 1], [5, 9, 9], [6, 10, 10], [0, 1, 1])
    assert order.tolist() == [1, 2, 0] and info == {"sites": 3, "descents": 1, "equal": 1, "passes": 3}


def build_native(tmp_path, name, *flags):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.fail("g++ is needed for tests/native/sites_sort_main.cpp")
    exe = tmp_path / name
    r = subprocess.run([gxx, "-g", "-std=c++17", "-Wall", *flags, "-o", str(exe), str(ROOT / "tests" / "native" / "sites_sort_main.cpp")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def test_native_program_plain(tmp_path):
    r = subprocess.run([str(build_native(tmp_path, "sites_sort_main", "-O2"))], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "sites sort ok" in r.stdout, r.stdout[-1500:] + r.stderr[-3000:]


def test_native_program_under_address_and_ub_sanitizers(tmp_path):
    """A stand-alone program (its own main, run directly): the serial forms over every size and pattern, every array in a
    heap block of exactly its length, built with -fsanitize=address,undefined."""
    exe = build_native(tmp_path, "sites_sort_main_san", "-O1", "-fsanitize=address,undefined", "-fno-omit-frame-pointer")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600,
                       env={"UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1", "ASAN_OPTIONS": "abort_on_error=1"})
    assert r.returncode == 0 and "sites sort ok" in r.stdout, r.stdout[-1500:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]


def test_symbols_and_documents():
    import alphabeta_rs_amd as abn

    header = (ROOT / "include" / "abneutral.h").read_text()
    doc = (ROOT / "INTEGRATION.md").read_text()
    Lib = abn.load_library(build_if_missing=True)
    for name in NEW_SYMBOLS:
        assert name in abn.EXPORTED_SYMBOLS and f"{name}(" in header and f"{name}(" in doc
        assert getattr(Lib, name).argtypes is not None
    for method in ("sort", "sort_order", "sort_info"):
        assert callable(getattr(abn.Sites, method))
    assert callable(abn.Context.sort_sites) and callable(abn.sort_sites_host)
    from alphabeta_rs_amd import build as B

    assert B.CSRC / "abn_sites_sort.hip" in B.SOURCES
