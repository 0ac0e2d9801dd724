"""The observation step and the state census in their host forms (alphabeta_rs_amd/csrc/abn_sim.hpp, abn_packed_census.hpp
through the two libraries) against the numpy model of tests/_sim_obs_model.py, which never calls the code under test: the
serial form and the walk of the kernel's lane function bit for bit, the thresholds from miscall and dropout probabilities,
the census against numpy, the native program plain and under the address and undefined-behaviour sanitizers, the symbols
and documents, and the statistics of the serial form against the probabilities its thresholds were made from."""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import _sim_model as M
import _sim_obs_model as O

ROOT = Path(__file__).resolve().parent.parent
NEW_SYMBOLS = ["abn_sim_obs_thresholds", "abn_sim_observe", "abn_sim_observe_dev", "abn_sim_study", "abn_packed_census_windows",
               "abn_packed_census_windows_dev"]
SEED = 0x9E3779B97F4A7C15
CUTS = (0, 1, 15, 16, 17, 255, 256, 257, 32_767, 32_768, 32_769)


@pytest.fixture(scope="module")
def S():
    from alphabeta_rs_amd import simulate

    return simulate


@pytest.fixture(scope="module")
def Cn():
    from alphabeta_rs_amd import census

    return census


def census_windows(L):
    """(begin, end) of the windows the census is held to on rows of L sites: every pair of CUTS and L, an empty window, two
    overlapping ones, one spanning three chunks"""
    cuts = [c for c in CUTS if c <= L] + [L]
    begin, end = [], []
    for b in cuts:
        for e in cuts:
            if b <= e:
                begin.append(b), end.append(e)
    for b, e in ((100, 100), (1000, 40_000), (30_000, 50_000), (300, 68_000)):
        if e <= L:
            begin.append(b), end.append(e)
    return begin, end


def test_serial_form_equals_the_model(S):
    rng = np.random.default_rng(21)
    for rows in (1, 8):
        nodes = [(5 * r + 2) % 11 for r in range(rows)]                       # not the identity
        for L in M.SIZES:
            fields = rng.integers(0, 4, size=(rows, L), dtype=np.uint8)       # fields of 3 inside the rows too
            packed = M.pack(fields)
            for othr in (O.obs_thresholds(*O.noise(0.05, 0.1)), O.random_othr(rng)):
                want = O.observe(SEED, packed, nodes, othr, L)
                assert np.array_equal(S.observe_host(SEED, packed, nodes, O.as_array(othr), L), want), (rows, L)
                assert np.array_equal(S.observe_host(SEED, packed, nodes, O.as_array(othr), L, in_place=True), want), (rows, L)
                for blocks, lazy in ((1, True), (3, True), (2, False)):
                    got = S.observe_host(SEED, packed, nodes, O.as_array(othr), L, walk_blocks=blocks, lazy=lazy)
                    assert np.array_equal(got, want), (rows, L, blocks, lazy)
            wide = S.observe_host(SEED, packed, nodes, O.as_array(othr), L, out_stride=M.row_stride(L) + 64)
            assert np.array_equal(wide[:, :M.row_stride(L)], want) and not wide[:, M.row_stride(L):].any()
            assert (O.unpack(want, L)[fields == 3] == 3).all()


def test_obs_thresholds_equal_the_model(abn, S):
    identity = np.eye(3)
    cases = [(identity, [0.0, 0.0, 0.0]), (identity, [1.0, 1.0, 1.0]), (identity, [0.0, 0.5, 1.0]), O.noise(0.05, 0.1), O.noise(0.0, 0.1),
             O.noise(1.0, 0.0), ([[0.2, 0.3, 0.5], [0.0, 0.0, 1.0], [1.0, 0.0, 0.0]], [0.25, 0.0, 0.75])]
    rng = np.random.default_rng(4)
    for _ in range(20):
        m = rng.random((3, 3))
        m[:, 2] = 0.0
        m /= 2.0 * m.sum(axis=1, keepdims=True)                                # the first two: at most 1 / 2 together
        m[:, 2] = 1.0 - (m[:, 0] + m[:, 1])
        if all(abs((row[0] + row[1]) + row[2] - 1.0) <= 1e-12 for row in m.tolist()):
            cases.append((m, rng.random(3)))
    for miscall, dropout in cases:
        got = S.obs_thresholds(miscall, dropout)
        assert got.tolist() == O.obs_thresholds(np.asarray(miscall).tolist(), list(dropout)), (miscall, dropout)
        assert (got[:, 0] <= got[:, 1]).all() and (got[:, 1] <= got[:, 2]).all()
    assert S.obs_thresholds(identity, [0.0] * 3).tolist() == [[M.MAX64] * 3, [0, M.MAX64, M.MAX64], [0, 0, M.MAX64]]
    assert S.obs_thresholds(identity, [1.0] * 3).tolist() == [[0, 0, 0]] * 3

    def refused(words, miscall=identity, dropout=(0.0, 0.0, 0.0)):
        with pytest.raises(abn.AbnError) as e:
            S.obs_thresholds(miscall, list(dropout))
        assert e.value.status == 1 and words in str(e.value), str(e.value)

    off = identity.copy()
    off[1] = [1e-9, 1.0, 0.0]                                                  # sums to 1 + 1e-9
    refused("miscall[1] does not sum to 1", miscall=off)
    for value in (-1e-9, 1.0 + 1e-9, float("nan"), float("inf")):
        bad = identity.copy()
        bad[2, 0] = value
        refused("lie in [0, 1]", miscall=bad)
        refused("lie in [0, 1]", dropout=(0.0, value, 0.0))
    import ctypes as C

    text = C.create_string_buffer(256)
    assert abn.load_library().abn_sim_obs_thresholds(None, None, None, text, 256) == 1 and b"null pointer" in text.value


def test_refusals_of_the_host_form(abn, S):
    othr = O.as_array(O.obs_thresholds(*O.noise(0.05, 0.1)))
    packed = M.pack(np.zeros((2, 100), dtype=np.uint8))

    def refused(words, **change):
        args = dict(seed=1, packed=packed, nodes=[0, 5], othr=othr, n_sites=100)
        with pytest.raises(abn.AbnError) as e:
            S.observe_host(**{**args, **change})
        assert e.value.status == 1 and words in str(e.value), str(e.value)

    assert S.observe_host(1, packed, [0, 5], othr, 100).shape == (2, 64)
    assert S.observe_host(1, np.zeros((2, 0), dtype=np.uint8), [0, 5], othr, 0).shape == (2, 0)
    refused("node_of_row[1] lies outside 0..65534", nodes=[0, 65535])
    refused("node_of_row[0] lies outside 0..65534", nodes=[-1, 0])
    bad = othr.copy()
    bad[1] = (5, 4, 9)
    refused("othr[1] decreases", othr=bad)
    refused("n_sites below 0 or above 2^34", n_sites=-1)
    refused("row_stride", n_sites=257)
    refused("row_stride", out_stride=96)
    refused("fewer than one row", packed=packed[:0], nodes=[])


def test_census_host_forms_equal_numpy(Cn):
    rng = np.random.default_rng(8)
    L = 70_001
    for n in (9, 1, 2):
        fields = rng.integers(0, 4, size=(n, L), dtype=np.uint8)
        fields[:, 40_000:41_000] = 3                                           # a wholly filtered window
        packed = M.pack(fields, stride=M.row_stride(L) + 128, fill=0x5A)
        begin, end = census_windows(L)
        begin, end = begin + [40_000], end + [41_000]
        want = O.census(fields, begin, end)
        assert np.array_equal(Cn.census_windows_host(packed, L, begin, end), want), n
        for chunk in (32_768, 256):
            assert np.array_equal(Cn.census_windows_host(packed, L, begin, end, walk_chunk=chunk), want), (n, chunk)
        assert not want[-1].any() and not want[begin.index(100)].any()
    assert Cn.census_windows_host(packed, L, [], []).shape == (0, 2, 3)


def build_native(tmp_path, name, *flags):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.fail("g++ is needed for tests/native/sim_study_main.cpp")
    exe = tmp_path / name
    r = subprocess.run([gxx, "-g", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", *flags, "-o", str(exe),
                        str(ROOT / "tests" / "native" / "sim_study_main.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def test_native_program_plain(tmp_path):
    r = subprocess.run([str(build_native(tmp_path, "sim_study_main", "-O2"))], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "sim study ok" in r.stdout, r.stdout[-1500:] + r.stderr[-3000:]


def test_native_program_under_address_and_ub_sanitizers(tmp_path):
    """A stand-alone program (its own main, run directly): the walk of the observation kernel's lane function and of the
    census kernels' job structure against the serial forms, every array in a heap block of exactly its length, built with
    -fsanitize=address,undefined."""
    exe = build_native(tmp_path, "sim_study_main_san", "-O1", "-fsanitize=address,undefined", "-fno-omit-frame-pointer")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600,
                       env={"UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1", "ASAN_OPTIONS": "abort_on_error=1"})
    assert r.returncode == 0 and "sim study ok" in r.stdout, r.stdout[-1500:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]


def test_statistics_of_the_host_form(S):
    """One row of L = 200 000 sites, true states drawn with p = [0.5, 0.2, 0.3], E = 0.05, F = 0.1.  Of the n_s sites of a
    true state s, each is observed as o with probability p(s, o) = 0.9 (0.95 if o = s else 0.025), or filtered with 0.1,
    independently: the cell count is binomial(n_s, p) with standard deviation sqrt(n_s p (1 - p)).  Every cell lies within
    six of these (and 1 for the thresholds' truncation to integers) of n_s p; a miss is a bug, not luck."""
    L, E, F = 200_000, 0.05, 0.1
    founder = M.as_array([[M.thresholds_of_row([0.5, 0.2])] * 3])
    truth = M.states(20260101, [-1], founder.tolist(), L)
    othr = S.obs_thresholds(*O.noise(E, F))
    assert othr.tolist() == O.obs_thresholds(*O.noise(E, F))
    seen = O.unpack(S.observe_host(20260101, M.pack(truth), [0], othr, L), L)[0]
    assert np.array_equal(seen, O.observe_fields(20260101, truth, [0], othr.tolist())[0])
    for s in range(3):
        n_s = int((truth[0] == s).sum())
        assert abs(n_s - L * (0.5, 0.2, 0.3)[s]) <= 6.0 * np.sqrt(L * 0.25)
        for o in range(4):
            p = F if o == 3 else (1.0 - F) * (1.0 - E if o == s else 0.5 * E)
            count = int(((truth[0] == s) & (seen == o)).sum())
            assert abs(count - n_s * p) <= 6.0 * np.sqrt(n_s * p * (1.0 - p)) + 1.0, (s, o, count, n_s * p)


def test_symbols_and_documents():
    import alphabeta_rs_amd as abn

    header = (ROOT / "include" / "abneutral.h").read_text()
    doc = (ROOT / "INTEGRATION.md").read_text()
    Lib = abn.load_library(build_if_missing=True)
    for name in NEW_SYMBOLS:
        assert name in abn.EXPORTED_SYMBOLS and f"{name}(" in header and f"{name}(" in doc
        assert getattr(Lib, name).argtypes is not None
    from alphabeta_rs_amd import census as Cn
    from alphabeta_rs_amd import simulate as S

    for function in ("obs_thresholds", "observe", "observe_dev", "observe_host", "study"):
        assert callable(getattr(S, function))
    for function in ("census_windows", "census_windows_dev", "census_windows_host"):
        assert callable(getattr(Cn, function))
    from alphabeta_rs_amd import build as B

    assert B.CSRC / "abn_packed_census.hpp" in B.DEPS and B.CSRC / "abn_pairwise.hip" in B.SOURCES
    assert "kTagObs = 6u" in (B.CSRC / "abn_philox.h").read_text() and "kTagObs = 6u" in header
    for text in ((ROOT / "README.md").read_text(), (ROOT / "DESIGN.md").read_text()):
        assert "abn_packed_census.hpp" in text and "--sim-replicates" in text
    assert "Replicate studies and the observation step" in (ROOT / "DESIGN.md").read_text()
    assert "## Simulation studies" in (ROOT / "docs" / "experiments.md").read_text()
    H = abn.load_host_library()
    assert hasattr(H, "abn_sim_observe_host") and hasattr(H, "abn_packed_census_windows_host")
