"""The union step (alphabeta_rs_amd/csrc/abn_sites_union.hpp) in its serial form, through the host shim: every site's union
rank, n_union and the gathered rows with their placeholders against the definition spelled out with sets and a sort in
tests/_union_model.py, and every refusal with its sample, site and text.  The lane functions the serial form calls pass by
pass are the ones the kernels run."""
import ctypes as C
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import _common_model as X
import _union_model as U
import _windows_model as M


@pytest.fixture(scope="module")
def L():
    L = M.hostlib()
    ll = C.c_longlong
    p = C.POINTER
    L.abh_sites_union_serial.argtypes = [C.c_int, p(ll), p(C.c_int), p(C.c_uint), p(C.c_uint), p(C.c_ubyte), p(C.c_uint), p(ll),
                                         C.c_char_p, ll, ll, p(C.c_ubyte), p(C.c_double), p(C.c_int), p(C.c_uint), p(C.c_uint),
                                         p(C.c_ubyte), p(C.c_ubyte), p(C.c_double)]
    L.abh_sites_union_serial.restype = ll
    return L


def serial(L, samples, gather=None):
    """-> ("ok", dest per sample, n_union[, gathered]) or ("refused", kind, sample, site, text).  gather: (n_union, code,
    level) — the codes and levels of the concatenated sites; gathered = the six arrays of n x n_union sites"""
    off, chrom, start, end, strand = X.concat(samples)
    t = L.abh_sites_union_serial.argtypes
    S, n = int(off[-1]), len(samples)
    dest = np.full(max(S, 1), 0xdeadbeef, dtype=np.uint32)
    refusal = np.zeros(3, dtype=np.int64)
    text = C.create_string_buffer(256)
    args = [n, off.ctypes.data_as(t[1]), chrom.ctypes.data_as(t[2]), start.ctypes.data_as(t[3]), end.ctypes.data_as(t[4]),
            strand.ctypes.data_as(t[5]), dest.ctypes.data_as(t[6]), refusal.ctypes.data_as(t[7]), text, len(text)]
    out = None
    if gather is None:
        args += [0] + [None] * 8
    else:
        nu, code, level = gather
        A = max(n * nu, 1)
        out = (np.full(A, -7, dtype=np.int32), np.full(A, 7, dtype=np.uint32), np.full(A, 7, dtype=np.uint32),
               np.full(A, 7, dtype=np.uint8), np.full(A, 7, dtype=np.uint8), np.full(A, 7.0))
        args += [nu, code.ctypes.data_as(t[11]), level.ctypes.data_as(t[12])] + [a.ctypes.data_as(ty) for a, ty in zip(out, t[13:])]
    got = L.abh_sites_union_serial(*args)
    if got < 0:
        assert got == -1 and refusal[0] > 0, got
        return ("refused", int(refusal[0]), int(refusal[1]), int(refusal[2]), text.value.decode())
    assert refusal.tolist() == [0, -1, -1] and text.value == b""
    res = ("ok", [dest[off[s]:off[s + 1]] for s in range(n)], got)
    return res + (tuple(a[:n * got].reshape(n, got) for a in out),) if gather is not None else res


def assert_same(got, want, name):
    assert got[0] == want[0] == "ok", (name, got[:4], want[:4])
    assert got[2] == want[2], (name, got[2], want[2])
    for g, w in zip(got[1], want[1]):
        assert g.dtype == w.dtype and g.tobytes() == w.tobytes(), name


def assert_gathered(L, samples, want, name):
    """the serial gather on codes i % 3 | 0x40 and levels i + 0.5 of the concatenated sites: own sites copied, placeholders
    with the union key, code 0x80 and level +0.0"""
    S, nu = sum(map(len, samples)), want[2]
    code = (np.arange(S) % 3 | 0x40).astype(np.uint8)
    level = np.arange(S) + 0.5
    got = serial(L, samples, gather=(nu, np.resize(code, max(S, 1)), np.resize(level, max(S, 1))))
    assert_same(got, want, name)
    off = np.concatenate([[0], np.cumsum([len(s) for s in samples])])
    for s, row in enumerate(U.padded(samples, want[3])):
        for j, col in enumerate(zip(*[k for k, _ in row])) if row else ():
            assert got[3][j][s].tolist() == list(col), (name, s, j)
        mine = [i for _, i in row]
        assert got[3][4][s].tolist() == [U.PLACEHOLDER_CODE if i is None else int(code[off[s] + i]) for i in mine], (name, s)
        want_level = np.array([0.0 if i is None else level[off[s] + i] for i in mine])
        assert got[3][5][s].tobytes() == want_level.tobytes(), (name, s)           # +0.0, bit for bit


def test_ranks_count_and_rows_against_the_sorted_set(L):
    seen = np.zeros(5, dtype=np.int64)
    cases = 0
    for name, samples, total in U.generated_cases():
        want = U.model(samples)
        assert want[0] == "ok", (name, want)                                        # none is skipped as refused
        assert_same(serial(L, samples), want, name)
        lonely_keys = len({k for s in samples for k in s if k[0] == 30})
        assert want[2] == total + lonely_keys, name
        if want[2] <= 300:
            assert_gathered(L, samples, want, name)
        seen += U.coverage(samples, want[3])
        cases += 1
    assert cases == 108
    assert seen.min() >= 5, dict(zip(("last only", "second group", "no site", "first", "last"), seen.tolist()))


def test_edges(L):
    key = lambda i, c=1: (c, 10 + i, 11 + i, i % 3)
    big = [key(i) for i in range(3000)]
    edge = [key(i, 1) for i in range(256)] + [key(i, 2) for i in range(300)]          # a run boundary on site 256
    other = [key(i, 1) for i in range(0, 400, 2)] + [key(i, 2) for i in range(1, 500)]
    for name, samples, n_union in (
            ("one sample", [big[:300]], 300),
            ("one empty sample", [[]], 0),
            ("empty samples alone", [[], [], []], 0),
            ("an empty sample among others", [big[:10], [], big[5:15]], 15),
            ("an empty first sample", [[], big[:10]], 10),
            ("disjoint", [big[:100], big[100:200]], 200),
            ("disjoint, interleaved", [big[0:200:2], big[1:200:2]], 200),
            ("identical", [big[:257], big[:257], big[:257]], 257),
            ("1 and 3000", [[big[1234]], big], 3000),
            ("3000 and 1 below all", [big, [(1, 5, 5, 0)]], 3001),
            ("only end differs", [[(1, 5, 6, 0), (1, 5, 7, 0)], [(1, 5, 7, 0)]], 2),
            ("only strand differs", [[(1, 5, 6, 0), (1, 5, 6, 2)], [(1, 5, 6, 1), (1, 5, 6, 2)]], 3),
            ("only the chromosome differs", [[(1, 5, 6, 0)], [(2, 5, 6, 0)]], 2),
            ("a chromosome only the last sample has", [big[:50], big[:50], big[:40] + [key(i, 2) for i in range(9)]], 59),
            ("a run boundary on site 256", [edge, other + [key(0, 3)]], 328 + 500 + 1),
            ("a run boundary on site 256, the second sample's", [other[:100], edge], len(set(other[:100]) | set(edge))),
            ("runs 1, 10, 2 with organelles", [[key(0, 1), key(0, 10), key(0, 2), key(0, 256), key(0, 257)],
                                                [key(0, 1), key(1, 10), key(0, 2), key(0, 257)]], 6)):
        want = U.model(samples)
        assert want[0] == "ok" and want[2] == n_union, (name, want[:3:2])
        assert_gathered(L, samples, want, name)
    got = serial(L, [big[:257]] * 3)                                                 # identical: dest is the identity
    assert all(d.tolist() == list(range(257)) for d in got[1]) and got[2] == 257


def test_every_refusal(L):
    rng = np.random.default_rng(7)
    kinds = {U.SPLIT: 0, U.NOT_ASCENDING: 0, U.RUN_ORDER: 0}
    for name, samples, kind in X.refusal_cases(rng):                                # the well-ordering's, texts unchanged
        if kind not in (X.SPLIT, X.NOT_ASCENDING):
            continue
        want = U.model(samples)
        got = serial(L, samples)
        assert want[:2] == ("refused", kind) and got[:4] == want, (name, got, want)
        assert got[4].startswith(f"sample {want[2]}, site {want[3]}: {X.WORDS[kind]}"), (name, got[4])
        kinds[kind] += 1
    for name, samples, sample, site in U.run_order_cases():
        want = U.model(samples)
        got = serial(L, samples)
        assert want == ("refused", U.RUN_ORDER, sample, site), (name, want)
        assert got[:4] == want, (name, got, want)
        assert got[4].startswith(f"sample {sample}, site {site}: run order"), (name, got[4])
        kinds[U.RUN_ORDER] += 1
    assert min(kinds.values()) >= 3, kinds
    # the well-ordering is judged first: its lowest site of the whole input, whatever the run order says
    a = [(2, 1, 1, 0), (1, 5, 6, 0), (1, 4, 6, 0)]
    assert serial(L, [[(1, 1, 1, 0), (2, 1, 1, 0)], a])[:4] == ("refused", U.NOT_ASCENDING, 1, 2)
    b = [(1, 5, 6, 0), (2, 1, 1, 0), (1, 9, 9, 0), (1, 9, 9, 0)]
    assert serial(L, [b])[:4] == U.model([b]) == ("refused", U.SPLIT, 0, 2)
    for bad in ((258, 1, 1, 0), (-1, 1, 1, 0), (1, 1, 1, 3)):                       # no index into the table of runs
        got = serial(L, [[(1, 1, 1, 0)], [(1, 1, 1, 0), bad]])
        assert got[:4] == ("refused", U.BAD_KEY, 1, 1), got
        assert "a chromosome outside 0..257, or a strand above 2" in got[4]


def test_serial_form_under_address_and_ub_sanitizers(tmp_path):
    """A stand-alone program (its own main, run directly): the serial step over seeded samples, empty ones included, every
    array in a heap block of exactly its length, against a union by sorted merge written out there, built with
    -fsanitize=address,undefined."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.fail("g++ is needed for the sanitizer build of tests/native/union_main.cpp")
    root = Path(__file__).resolve().parent.parent
    exe = tmp_path / "union_main"
    r = subprocess.run([gxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-o",
                        str(exe), str(root / "tests" / "native" / "union_main.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600,
                       env={"UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1", "ASAN_OPTIONS": "abort_on_error=1"})
    assert r.returncode == 0 and "sanitized union sites ok" in r.stdout, r.stdout[-1500:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
