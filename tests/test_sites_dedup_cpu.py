"""The collapse of repeated sites in its serial forms (alphabeta_rs_amd/csrc/abn_sites_dedup.hpp through host_capi.cpp)
against the numpy / Python model of tests/_dedup_model.py, which never calls the code under test: the serial form under all
four policies, the walk of the kernels' structure — flags lane by lane, BEST's walk from the head's lane, tile counts,
scan, scatter — the refusals, and the native program plain and under the address and undefined-behaviour sanitizers."""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import _dedup_model as M

ROOT = Path(__file__).resolve().parent.parent
NEW_SYMBOLS = ["abn_sites_dedup", "abn_sites_dedup_order", "abn_sites_dedup_info", "abn_sites_dedup_keys",
               "abn_sites_dedup_keys_dev"]


@pytest.fixture(scope="module")
def L():
    return M.hostlib()


def test_sizes_and_patterns(L):
    assert L.abh_sites_sort_tile() == M.TILE and M.SIZES == (0, 1, 2, 63, 64, 65, 2047, 2048, 2049, 3 * 2048 + 17)
    names = {name for n in M.SIZES for name, _ in M.patterns(n, seed=n)}
    assert names == {"no repeats", "all equal", "pairs", "random runs", "all-NaN runs", "straddling", "start and end",
                     "long run"}
    for n in M.SIZES:
        for name, r in M.patterns(n, seed=n):
            assert len(r[0]) == n and M.first_descent(r) == -1, (n, name)
    n, r = 3 * M.TILE + 17, dict(M.patterns(3 * M.TILE + 17, seed=5))
    ids, _ = M.run_ids(r["long run"])
    assert np.bincount(ids).max() == M.LONG_RUN == 2 * 2048 + 5
    ids, _ = M.run_ids(r["straddling"])
    heads = np.flatnonzero(np.bincount(ids)[ids] == 2)[::2]
    assert heads[:3].tolist() == [63, 127, 191] and (heads % 64 == 63).all()
    pm = r["random runs"][4]
    assert np.isnan(pm).any() and (np.signbit(pm) & (pm == 0)).any() and (~np.signbit(pm) & (pm == 0)).any()


def test_better_is_the_stated_rule():
    nan = float("nan")
    assert M.better(0.5, 0.4) and not M.better(0.4, 0.5) and not M.better(0.5, 0.5)       # ties keep the earlier record
    assert not M.better(-0.0, 0.0) and not M.better(0.0, -0.0)                            # the zeros tie
    assert M.better(0.1, nan) and not M.better(nan, 0.1) and not M.better(nan, nan)       # a run of NaN keeps its first


def test_serial_form_equals_the_model(L):
    for n in M.SIZES:
        for name, r in M.patterns(n, seed=n):
            for policy in M.POLICIES:
                want, info = M.model(r, policy)
                rc, order, got, descent = M.host_dedup(L, r, policy)
                assert rc == 0 and descent == -1, (n, name, policy)
                assert np.array_equal(order, want) and got == info, (n, name, policy)
                if name == "no repeats":
                    assert np.array_equal(order, np.arange(n)) and info[2:] == [0, 0]
                if name == "all equal" and n > 1:
                    assert info[1] == (0 if policy == "drop" else 1) and info[2] == 1


def test_walk_of_the_kernels_equals_the_model(L):
    for n in M.SIZES:
        for name, r in M.patterns(n, seed=100 + n):
            for policy in M.POLICIES:
                want, info = M.model(r, policy)
                for blocks in (1, 3):                                         # every lane strides; three workgroups interleave
                    rc, order, got, check = M.host_dedup(L, r, policy, walk_blocks=blocks)
                    assert rc == 0 and np.array_equal(order, want) and got == info, (n, name, policy, blocks)
                    assert check == [-1, 0, info[2], info[3]], (n, name, policy, blocks)


def test_flags_find_the_first_descent_and_the_bad_keys(L):
    r = [a.copy() for a in dict(M.patterns(3 * M.TILE + 17, seed=9))["random runs"]]
    for at in (M.TILE + 1, 5000):                                             # two descents: the first is reported
        r[1][at] = 0
    assert M.first_descent(r) == M.TILE + 1
    for policy in M.POLICIES:
        rc, _, _, descent = M.host_dedup(L, r, policy)
        assert rc == 1 and descent == M.TILE + 1, policy
        _, _, _, check = M.host_dedup(L, r, policy, walk_blocks=3)
        assert check[0] == M.TILE + 1 and check[1] == 0, policy
    r[0][7] = 300
    r[3][9] = 3
    _, _, _, check = M.host_dedup(L, r, "first", walk_blocks=2)
    assert check[1] == 2


def test_host_form_refusals(L):
    import alphabeta_rs_amd as abn
    from alphabeta_rs_amd import dedup as D

    one = M.records([1, 1], [5, 5], [6, 6], [0, 0], [0.5, 0.7], [0, 2])
    for bad in ((258, 0, 0, 0), (-1, 0, 0, 0), (0, 0, 0, 3)):                 # a key outside its ranges
        r = M.records(*([0, v] for v in bad), [0.5, 0.5], [0, 0])
        rc, _, _, descent = M.host_dedup(L, r, "first")
        assert rc == 1 and descent == -1, bad
        with pytest.raises(abn.AbnError):
            D.dedup_sites_host(*r)
    down = M.records([1, 1, 0], [5, 5, 9], [6, 6, 10], [0, 0, 0], [0.5, 0.5, 0.5], [0, 0, 0])
    rc, _, _, descent = M.host_dedup(L, down, "best")
    assert rc == 1 and descent == 2
    with pytest.raises(abn.AbnError) as e:
        D.dedup_sites_host(*down, policy="best")
    assert "site 2" in str(e.value) and "sort first" in str(e.value)
    for policy in (-1, 4):
        assert M.host_dedup(L, one, policy)[0] == 1
    with pytest.raises(ValueError):
        D.dedup_sites_host(*one, policy="newest")
    order, info = np.zeros(2, dtype=np.int64), np.zeros(4, dtype=np.int64)
    ptrs = [a.ctypes.data for a in one]
    assert L.abn_sites_dedup_keys_host(1 << 32, *ptrs, 0, order.ctypes.data, info.ctypes.data, None) == 1
    assert L.abn_sites_dedup_keys_host(-1, *ptrs, 0, order.ctypes.data, info.ctypes.data, None) == 1
    assert L.abn_sites_dedup_keys_host(2, *ptrs, 0, order.ctypes.data, None, None) == 1
    for k in range(6):
        nulled = list(ptrs)
        nulled[k] = None
        assert L.abn_sites_dedup_keys_host(2, *nulled, 0, order.ctypes.data, info.ctypes.data, None) == 1, k
    assert L.abn_sites_dedup_keys_host(2, *ptrs, 0, None, info.ctypes.data, None) == 1
    assert L.abn_sites_dedup_keys_host(0, *[None] * 6, 0, None, info.ctypes.data, None) == 0 and info.tolist() == [0, 0, 0, 0]
    order, info = D.dedup_sites_host(*one, policy="best")
    assert order.tolist() == [1] and info == {"sites": 2, "kept": 1, "repeated": 1, "disagreeing": 1}
    assert D.dedup_sites_host(*one, policy=D.dedup.__defaults__[0])[0].tolist() == [0]       # the default: first
    assert D.dedup_sites_host(*one, policy="drop")[0].tolist() == []


def build_native(tmp_path, name, *flags):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.fail("g++ is needed for tests/native/sites_dedup_main.cpp")
    exe = tmp_path / name
    r = subprocess.run([gxx, "-g", "-std=c++17", "-Wall", *flags, "-o", str(exe), str(ROOT / "tests" / "native" / "sites_dedup_main.cpp")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def test_native_program_plain(tmp_path):
    r = subprocess.run([str(build_native(tmp_path, "sites_dedup_main", "-O2"))], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "sites dedup ok" in r.stdout, r.stdout[-1500:] + r.stderr[-3000:]


def test_native_program_under_address_and_ub_sanitizers(tmp_path):
    """A stand-alone program (its own main, run directly): the serial form and the walk of the kernels' structure over every
    size, pattern and policy, every array in a heap block of exactly its length, built with -fsanitize=address,undefined."""
    exe = build_native(tmp_path, "sites_dedup_main_san", "-O1", "-fsanitize=address,undefined", "-fno-omit-frame-pointer")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600,
                       env={"UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1", "ASAN_OPTIONS": "abort_on_error=1"})
    assert r.returncode == 0 and "sites dedup ok" in r.stdout, r.stdout[-1500:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]


def test_symbols_and_documents():
    import alphabeta_rs_amd as abn

    header = (ROOT / "include" / "abneutral.h").read_text()
    doc = (ROOT / "INTEGRATION.md").read_text()
    Lib = abn.load_library(build_if_missing=True)
    for name in NEW_SYMBOLS:
        assert name in abn.EXPORTED_SYMBOLS and f"{name}(" in header and f"{name}(" in doc
        assert getattr(Lib, name).argtypes is not None
    for k, name in enumerate(("FIRST", "LAST", "BEST", "DROP")):
        assert f"#define ABN_DEDUP_{name} {k}\n" in header
    from alphabeta_rs_amd import dedup as D

    for function in ("dedup", "dedup_order", "dedup_info", "dedup_sites", "dedup_sites_host"):
        assert callable(getattr(D, function))
    assert D.POLICIES == ("first", "last", "best", "drop")
    from alphabeta_rs_amd import build as B

    assert B.CSRC / "abn_sites_dedup.hip" in B.SOURCES
    for text in ((ROOT / "README.md").read_text(), (ROOT / "DESIGN.md").read_text()):
        assert "abn_sites_dedup.hpp" in text and "--dedup" in text
