"""The simulated methylomes in their host forms (alphabeta_rs_amd/csrc/abn_sim.hpp through the two libraries) against the
numpy model of tests/_sim_model.py, which never calls the code under test: the serial form and the walk of the kernel's
lane structure bit for bit, the thresholds from rates against the oracle's matrix powers, the refusals by their messages,
the native program plain and under the address and undefined-behaviour sanitizers, and the statistics of the serial form
against the model's dt1t2 (oracle.divergence)."""
import ctypes as C
import shutil
import subprocess
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest

import _sim_model as M

ROOT = Path(__file__).resolve().parent.parent
NEW_SYMBOLS = ["abn_sim_thresholds", "abn_sim_grid", "abn_sim_codes", "abn_sim_codes_dev", "abn_sim_pedigree"]
FIXTURE_RATES = (3.974271e-09, 1.519045e-07)      # src/divergence.rs:146-147
SEED = 0x9E3779B97F4A7C15


@pytest.fixture(scope="module")
def S():
    from alphabeta_rs_amd import simulate

    return simulate


def walk(parent, thr, emit, n_sites, blocks, lazy, stride=None, fill=0xFF):
    """abh_sim_codes_walk: the kernel's lane structure on the host"""
    from alphabeta_rs_amd._ffi import load_host_library

    H = load_host_library()
    H.abh_sim_codes_walk.argtypes = [C.c_uint64, C.c_int] + [C.c_void_p] * 3 + [C.c_longlong, C.c_longlong, C.c_int, C.c_void_p,
                                                                                 C.c_longlong]
    parent, emit, thr = np.asarray(parent, dtype=np.int32), np.asarray(emit, dtype=np.uint8), M.as_array(thr)
    stride = M.row_stride(n_sites) if stride is None else stride
    out = np.full((int(emit.sum()), stride), fill, dtype=np.uint8)
    assert H.abh_sim_codes_walk(SEED, len(parent), parent.ctypes.data, thr.ctypes.data, emit.ctypes.data, n_sites, blocks, lazy,
                                out.ctypes.data, stride) == 0
    return out


def test_model_philox_is_the_oracles(oracle):
    key = (SEED & 0xFFFFFFFF, SEED >> 32)
    got = np.stack(M.philox([0, 1, 77, 0xFFFFFFFF], 1, 9, M.TAG_SIM, *key), axis=1)
    for k, c0 in enumerate([0, 1, 77, 0xFFFFFFFF]):
        assert np.array_equal(got[k], oracle.philox((c0, 1, 9, M.TAG_SIM), key))
    hi, lo = M.draw_words(SEED, 3, 10)
    assert hi[6] == oracle.philox((1, 0, 3, 5), key)[2] and lo[6] == oracle.philox((1, 1, 3, 5), key)[2]
    assert int(M.draws(SEED, 3, 10)[6]) == (int(hi[6]) << 32) | int(lo[6])


def test_model_pack_is_the_formats(abn):
    rng = np.random.default_rng(3)
    for L in (1, 17, 300):
        fields = rng.integers(0, 3, size=(3, L), dtype=np.uint8)
        assert np.array_equal(M.pack(fields), abn.pack_codes(fields))


def test_serial_form_equals_the_model(S):
    rng = np.random.default_rng(11)
    for name, parent, generation, emit in M.TREES:
        rates = S.thresholds(parent, generation, 0.1, 0.2, 0.7, 0.3)
        anything = M.random_thresholds(rng, len(parent))
        for L in M.SIZES:
            for thr in (rates.tolist(), anything):
                want = M.model(SEED, parent, thr, emit, L)
                assert np.array_equal(S.codes_host(SEED, parent, M.as_array(thr), emit, L), want), (name, L)
        wide = S.codes_host(SEED, parent, rates, emit, 257, row_stride=256)
        assert np.array_equal(wide[:, :128], M.model(SEED, parent, rates.tolist(), emit, 257)) and not wide[:, 128:].any(), name
    assert S.codes_host(SEED, [-1], M.as_array([[[0, 0]] * 3]), [1], 0).shape == (1, 0)


def test_walk_of_the_kernel_equals_the_model(S):
    rng = np.random.default_rng(12)
    for name, parent, generation, emit in M.TREES:
        thr = M.random_thresholds(rng, len(parent))
        for L in M.SIZES:
            want = M.model(SEED, parent, thr, emit, L, stride=M.row_stride(L) + 64, fill=0x5A)
            for blocks, lazy in ((1, 1), (3, 1), (2, 0)):
                got = walk(parent, thr, emit, L, blocks, lazy, stride=M.row_stride(L) + 64, fill=0x5A)
                assert np.array_equal(got, want), (name, L, blocks, lazy)


def test_planted_ties_in_the_walk(S):
    """a draw whose high word equals a threshold's: the low words decide, in the lazy walk as in the law"""
    for which in (0, 1):
        for delta in (-1, 0, 1):
            for state in (0, 1, 2):
                thr, wanted = M.planted(SEED, which, delta, state)
                st = M.states(SEED, [-1, 0], thr, 64)
                assert (st[0] == state).all() and st[1][37] == wanted, (which, delta, state)
                want = M.model(SEED, [-1, 0], thr, [1, 1], 64)
                for lazy in (1, 0):
                    assert np.array_equal(walk([-1, 0], thr, [1, 1], 64, 1, lazy), want), (which, delta, state, lazy)
                assert np.array_equal(S.codes_host(SEED, [-1, 0], M.as_array(thr), [1, 1], 64), want)


def test_transition_thresholds_are_the_oracles_rows(S, oracle):
    """for v > 0: thr is bit-equal to the thresholds of the rows of oracle.matrix_power(oracle.genmatrix(a, b), dt)"""
    values = (0.0, 1.0, 1e-3)
    pairs = [(a, b) for a in values for b in values] + [FIXTURE_RATES, (FIXTURE_RATES[0], 1e-3), (1e-3, FIXTURE_RATES[1])]
    for alpha, beta in pairs:
        G = oracle.genmatrix(alpha, beta)
        for dt in (0, 1, 2, 31, 127):
            got = S.thresholds([-1, 0, 1], [0, 0, dt], alpha, beta, 0.75, 0.5)
            P = oracle.matrix_power(G, dt)
            want = [M.thresholds_of_row(P[s]) for s in range(3)]
            assert got[2].tolist() == want, (alpha, beta, dt)
            assert got[1].tolist() == [[M.MAX64, M.MAX64], [0, M.MAX64], [0, 0]]          # power 0: the child copies its parent
            assert (got[:, :, 0] <= got[:, :, 1]).all()


def test_founder_thresholds_against_exact_arithmetic(S, oracle):
    """The founder's row is [p, w (1 - p), (1 - w)(1 - p)] . G^g0 (src/divergence.rs:44,55).  Taken exactly (Fraction) on
    the doubles the oracle holds — the three entries of the vector as the reference rounds them, the nine of the power —
    entry j is a sum of three products.  The code computes it in three fused steps from 0, each rounding a value that
    is at most 1 (a partial sum of a probability) to at most half an ulp, 2^-54: |p_j - exact_j| <= 3 * 2^-54.  c0 = p_0; c1 =
    p_0 + p_1 adds one rounded add, again of a value at most 1 (a sum that rounds to 1 or above becomes 2^64 - 1 on both
    sides): |c1 - exact| <= (3 + 3 + 1) * 2^-54.  Scaled by 2^64 and with the truncation to an integer, below 1: the
    thresholds differ from floor(exact * 2^64) by at most 3 * 2^10 + 1 and 7 * 2^10 + 1."""
    for alpha, beta in ((2e-3, 5e-3), FIXTURE_RATES, (0.1, 0.2), (1e-3, 1e-3)):
        for p, w in ((0.7, 0.3), (0.75, 0.06892953), (1.0, 0.5), (0.0, 1.0)):
            for g0 in (0, 1, 2, 31, 127):
                got = S.thresholds([-1], [g0], alpha, beta, p, w)[0]
                assert got[0].tolist() == got[1].tolist() == got[2].tolist()
                p_mm = 1.0 - p
                sv = [Fraction(p), Fraction(w * p_mm), Fraction((1.0 - w) * p_mm)]
                P = oracle.matrix_power(oracle.genmatrix(alpha, beta), g0)
                row = [sum(sv[i] * Fraction(float(P[i][j])) for i in range(3)) for j in range(3)]
                exact = [min(int(row[0] * (1 << 64)), M.MAX64), min(int((row[0] + row[1]) * (1 << 64)), M.MAX64)]
                assert abs(int(got[0][0]) - exact[0]) <= 3 * 2 ** 10 + 1, (alpha, beta, p, w, g0)
                assert abs(int(got[0][1]) - exact[1]) <= 7 * 2 ** 10 + 1, (alpha, beta, p, w, g0)
    assert S.thresholds([-1], [0], 0.1, 0.2, 0.7, 0.3)[0][0].tolist() == M.thresholds_of_row([0.7, 0.3 * (1.0 - 0.7)])


def test_refusals_by_their_messages(abn, S):
    thr = M.as_array([[[0, M.MAX64]] * 3] * 3)
    ok = dict(seed=1, parent=[-1, 0, 1], thr=thr, emit=[1, 0, 1], n_sites=100)

    def refused(words, **change):
        with pytest.raises(abn.AbnError) as e:
            S.codes_host(**{**ok, **change})
        assert e.value.status == 1 and words in str(e.value), str(e.value)

    assert S.codes_host(**ok).shape == (2, 64)
    refused("fewer than one node", parent=[], thr=thr[:0], emit=[])
    refused("parent[0] is not -1", parent=[0, 0, 1])
    refused("parent[1] is not a node in front of it", parent=[-1, 1, 0])
    refused("parent[2] is not a node in front of it", parent=[-1, 0, -1])
    bad = thr.copy()
    bad[1, 2] = (5, 4)
    refused("thr[1][2][0] lies above its [1]", thr=bad)
    refused("no emitted node", emit=[0, 0, 0])
    refused("n_sites below 0 or above 2^34", n_sites=-1)
    refused("n_sites below 0 or above 2^34", n_sites=(1 << 34) + 1, row_stride=64)
    refused("row_stride", row_stride=96)
    refused("row_stride", n_sites=257, row_stride=64)
    many = 65536
    with pytest.raises(abn.AbnError) as e:
        S.codes_host(1, [-1] + [0] * (many - 1), np.zeros((many, 3, 2), dtype=np.uint64), [1] * many, 1)
    assert "more than 65535 nodes" in str(e.value)
    from alphabeta_rs_amd._ffi import load_host_library

    H = load_host_library()
    text = C.create_string_buffer(256)
    assert H.abn_sim_codes_host(1, 3, None, thr.ctypes.data, None, 100, None, 64, text, 256) == 1 and b"null pointer" in text.value
    with pytest.raises(ValueError):
        S.codes_host(1, [-1, 0], thr, [1, 1], 10)                                           # three nodes' thresholds, two nodes

    def no_thresholds(words, parent=(-1, 0, 1), generation=(0, 1, 2), rates=(0.1, 0.2, 0.7, 0.3)):
        with pytest.raises(abn.AbnError) as e:
            S.thresholds(list(parent), list(generation), *rates)
        assert e.value.status == 1 and words in str(e.value), str(e.value)

    no_thresholds("generation[2] lies outside 0..127", generation=(0, 1, 128))
    no_thresholds("generation[0] lies outside 0..127", generation=(-1, 1, 2))
    no_thresholds("node 2 is older than its parent", generation=(0, 3, 2))
    no_thresholds("parent[0] is not -1", parent=(0, 0, 1))
    no_thresholds("parent[2] is not a node in front of it", parent=(-1, 0, 2))
    for k in range(4):
        for value in (-1e-9, 1.0 + 1e-9, float("nan"), float("inf")):
            rates = [0.1, 0.2, 0.7, 0.3]
            rates[k] = value
            no_thresholds("lie in [0, 1]", rates=rates)
    L = abn.load_library()
    assert L.abn_sim_thresholds(0.1, 0.2, 0.7, 0.3, 0, None, None, None, text, 256) == 1 and b"null pointer" in text.value
    assert S.thresholds([-1, 0], [127, 127], 0.0, 1.0, 1.0, 0.0).shape == (2, 3, 2)


def build_native(tmp_path, name, *flags):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.fail("g++ is needed for tests/native/sim_main.cpp")
    exe = tmp_path / name
    r = subprocess.run([gxx, "-g", "-std=c++17", "-Wall", *flags, "-o", str(exe), str(ROOT / "tests" / "native" / "sim_main.cpp")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def test_native_program_plain(tmp_path):
    r = subprocess.run([str(build_native(tmp_path, "sim_main", "-O2"))], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "sim ok" in r.stdout, r.stdout[-1500:] + r.stderr[-3000:]


def test_native_program_under_address_and_ub_sanitizers(tmp_path):
    """A stand-alone program (its own main, run directly): the serial form and the walk of the kernel's lane structure over
    every size and tree, every array in a heap block of exactly its length, built with -fsanitize=address,undefined."""
    exe = build_native(tmp_path, "sim_main_san", "-O1", "-fsanitize=address,undefined", "-fno-omit-frame-pointer")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600,
                       env={"UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1", "ASAN_OPTIONS": "abort_on_error=1"})
    assert r.returncode == 0 and "sim ok" in r.stdout, r.stdout[-1500:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]


def test_statistics_of_the_serial_form(S, oracle):
    """Every pair's D lies within 6 sqrt(dt1t2 / L) of the model's dt1t2: a site contributes |s_i - s_j| / 2 in {0, 1/2, 1},
    whose variance is at most its mean, so D's standard deviation is at most sqrt(dt1t2 / L); a miss at six of these is
    a bug, not luck."""
    parent, generation = M.TREE8
    alpha, beta, p_uu0, w, L = 2e-3, 5e-3, 0.7, 0.3, 100_000
    emit = [1] * 8
    thr = S.thresholds(parent, generation, alpha, beta, p_uu0, w)
    packed = S.codes_host(20260101, parent, thr, emit, L)
    import alphabeta_rs_amd as abn

    st = abn.unpack_codes(packed, L)
    assert st.max() <= 2 and np.array_equal(st, M.states(20260101, parent, thr.tolist(), L))
    rows, p0uu, _, _ = M.pedigree(st, parent, generation, emit)
    assert rows.shape == (28, 4)
    dt, _ = oracle.divergence(rows, 1.0 - p_uu0, p_uu0, alpha, beta, w)
    for r in range(28):
        assert abs(rows[r, 3] - dt[r]) <= 6.0 * np.sqrt(dt[r] / L), (rows[r], dt[r])
    assert rows[0].tolist()[:3] == [2.0, 2.0, 3.0] and rows[27].tolist()[:3] == [2.0, 9.0, 5.0]
    assert rows[18].tolist()[:3] == [3.0, 5.0, 8.0]                                   # nodes 3 and 4 split at node 1


def test_symbols_and_documents():
    import alphabeta_rs_amd as abn

    header = (ROOT / "include" / "abneutral.h").read_text()
    doc = (ROOT / "INTEGRATION.md").read_text()
    Lib = abn.load_library(build_if_missing=True)
    for name in NEW_SYMBOLS:
        assert name in abn.EXPORTED_SYMBOLS and f"{name}(" in header and f"{name}(" in doc
        assert getattr(Lib, name).argtypes is not None
    from alphabeta_rs_amd import simulate as S

    for function in ("thresholds", "codes", "codes_dev", "codes_host", "pedigree", "launch_grid"):
        assert callable(getattr(S, function))
    from alphabeta_rs_amd import build as B

    assert B.CSRC / "abn_sim.hip" in B.SOURCES and B.CSRC / "abn_sim.hpp" in B.DEPS
    philox = (B.CSRC / "abn_philox.h").read_text()
    assert "kTagSim = 5u" in philox
    for text in ((ROOT / "README.md").read_text(), (ROOT / "DESIGN.md").read_text()):
        assert "abn_sim.hpp" in text and "--simulate" in text
    assert "## Simulating methylomes" in (ROOT / "docs" / "experiments.md").read_text()
