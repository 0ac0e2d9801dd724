"""The pedigree build from resident sites (alphabeta_rs_amd/csrc/abn_codes.hpp) in its serial form, through the host shim:
the reduced merge, the pack of the merged bytes and the rc_meth_lvl fold of a sample against a Python model — the merge by
line number, abn_pack_codes of the code bytes, a float loop.  The index functions, the two predicates, the dword packer
and the `+0.0 for an uncounted site` form of the fold are the ones the kernels run; the chunk length is a parameter here,
a slab's line count on the device."""
import ctypes as C
import shutil
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

import _codes_model as K
import _windows_model as M

RECORD, ACCEPTED, REJECTED, NOTHING = 0, 1, 2, 3       # a line: a device record, deferred and a site, deferred and none, no site
CHUNK_LINES = (1, 2, 3, 64, 0)                          # 0: the whole file is one chunk
SITE_COUNTS = (0, 1, 15, 16, 17, 255, 256, 257)
NEG0 = struct.pack("<d", -0.0)


@pytest.fixture(scope="module")
def L():
    L = M.hostlib()
    ll, u32p, u8p, dp = C.c_longlong, C.POINTER(C.c_uint32), C.POINTER(C.c_uint8), C.POINTER(C.c_double)
    llp = C.POINTER(ll)
    L.abh_codes_build_serial.argtypes = [C.c_int, llp, llp, ll, u32p, u32p, dp, dp, ll, llp, u8p, dp, dp, C.c_double, ll,
                                         u8p, dp, u8p, dp, llp]
    L.abh_codes_build_serial.restype = C.c_int
    return L


def make_sample(rng, n_sites, pattern):
    """the lines of a file with exactly n_sites sites (line 0 is the header: no site): their class and, for the sites,
    status, posterior and level.  Inserted records sit at the edges of chunks of 2, 3 and 64 lines and next to each other."""
    n_lines = 1 + n_sites + int(rng.integers(0, 1 + n_sites // 4 + 2))
    kind = np.full(n_lines, NOTHING)
    site_lines = np.sort(rng.choice(np.arange(1, n_lines), size=n_sites, replace=False)) if n_sites else np.zeros(0, dtype=np.int64)
    kind[site_lines] = RECORD
    is_site = kind == RECORD
    at = np.arange(n_lines)
    if pattern == "edges":
        kind[is_site & ((at % 64 == 0) | (at % 64 == 63) | (at % 3 == 0) | (at % 2 == 1) & (at % 5 == 0))] = ACCEPTED
    elif pattern == "adjacent":
        for a in rng.integers(1, max(n_lines, 2), size=4):
            sel = at[(at >= a) & (at < a + 3) & is_site]
            kind[sel] = ACCEPTED
    elif pattern == "all_inserted":
        kind[is_site] = ACCEPTED
    elif pattern == "mixed":
        kind[is_site & (rng.random(n_lines) < 0.3)] = ACCEPTED
    kind[(kind == NOTHING) & (rng.random(n_lines) < 0.4)] = REJECTED
    kind[0] = NOTHING
    pm = np.where(rng.random(n_lines) < 0.4, K.FILTER, rng.random(n_lines))     # at the filter: counted, and not filtered
    pm[(kind == ACCEPTED) & (rng.random(n_lines) < 0.35)] = np.nan              # only the host's parser yields a NaN posterior
    ml = rng.random(n_lines)
    ml[rng.random(n_lines) < 0.25] = -0.0                                       # among the filtered and the counted sites
    if pattern == "neg_zero":
        ml[:] = -0.0
    return kind, {"status": rng.integers(0, 3, size=n_lines).astype(np.uint8), "pm": pm, "ml": ml}


def run(L, kind, f, chunk_lines, stride):
    n_lines = len(kind)
    chunk_lines = chunk_lines or n_lines
    rec = np.flatnonzero(kind == RECORD)
    ins = np.flatnonzero(kind == ACCEPTED).astype(np.int64)
    n_chunks = (n_lines + chunk_lines - 1) // chunk_lines
    lines = np.minimum(chunk_lines, n_lines - chunk_lines * np.arange(n_chunks)).astype(np.int64)
    count = np.bincount(rec // chunk_lines, minlength=n_chunks).astype(np.int64)
    col = lambda a, t: np.ascontiguousarray(a, dtype=t)
    meta = col(7 | 1 << 16 | f["status"][rec].astype(np.uint32) << 20 | np.uint32(1 << 24), np.uint32)   # the status among other bits
    total = len(rec) + len(ins)
    code, level = np.full(total, 0x55, dtype=np.uint8), np.full(total, -7.0)
    row = np.full(stride, 0x5a, dtype=np.uint8)
    s, k = C.c_double(-1.0), C.c_longlong(-1)
    t = L.abh_codes_build_serial.argtypes
    p = lambda a, ty: a.ctypes.data_as(ty)
    rc = L.abh_codes_build_serial(n_chunks, p(count, t[1]), p(lines, t[2]), 0, p(col(rec % chunk_lines, np.uint32), t[4]),
                                  p(meta, t[5]), p(col(f["pm"][rec], np.float64), t[6]), p(col(f["ml"][rec], np.float64), t[7]),
                                  len(ins), p(ins, t[9]), p(col(f["status"][ins], np.uint8), t[10]),
                                  p(col(f["pm"][ins], np.float64), t[11]), p(col(f["ml"][ins], np.float64), t[12]), K.FILTER,
                                  stride, p(code, t[15]), p(level, t[16]), p(row, t[17]), C.byref(s), C.byref(k))
    assert rc == 0
    return code, level, row, struct.pack("<d", s.value), k.value


def test_serial_build_against_the_python_model(abn, L):
    rng = np.random.default_rng(20261019)
    seen = {"inserted": 0, "nan_uncounted": 0, "neg0_counted": 0, "neg0_filtered": 0, "padded_rows": 0, "edge": 0, "adjacent": 0}
    patterns = ("none", "edges", "adjacent", "all_inserted", "mixed", "neg_zero")
    for case, n_first in enumerate(SITE_COUNTS * 3):
        pattern = patterns[case % len(patterns)]
        counts = [n_first] + [SITE_COUNTS[(case + 3 * j) % len(SITE_COUNTS)] for j in (1, 2)]   # samples of different length
        samples = [make_sample(rng, n, pattern if j == 0 else patterns[(case + j) % len(patterns)]) for j, n in enumerate(counts)]
        stride = max(abn.packed_row_stride(max(counts)), 64)
        model = []
        for kind, f in samples:
            merged = np.flatnonzero((kind == RECORD) | (kind == ACCEPTED))        # the Python merge: the sites by line number
            model.append((merged, K.code_bytes(f["status"][merged], f["pm"][merged]), K.counted(f["pm"][merged])))
        want_rows = K.packed_rows(abn, [m[1] for m in model], stride)
        for (kind, f), (merged, code, cnt), want_row, n in zip(samples, model, want_rows, counts):
            assert len(merged) == n
            want_sum, want_kept = K.fold(f["pm"][merged], f["ml"][merged])
            for chunk_lines in CHUNK_LINES:
                label = (case, pattern, n, chunk_lines)
                got_code, got_level, row, s, k = run(L, kind, f, chunk_lines, stride)
                assert got_code.tobytes() == (code | np.where(cnt, K.COUNTED, 0).astype(np.uint8)).tobytes(), label
                assert got_level.tobytes() == f["ml"][merged].tobytes(), label
                assert row.tobytes() == want_row.tobytes(), label                  # padding fields included
                assert (s, k) == (want_sum, want_kept), label
            ins = kind[merged] == ACCEPTED
            nan = np.isnan(f["pm"][merged])
            assert not (nan & ~ins).any()
            assert not (code[nan] & 0x80).any() and not cnt[nan].any()             # a NaN posterior: unflagged, and uncounted
            neg0 = np.array([struct.pack("<d", v) == NEG0 for v in f["ml"][merged]], dtype=bool)
            lines = merged[ins]
            seen["inserted"] += int(ins.sum())
            seen["nan_uncounted"] += int(nan.sum())
            seen["neg0_counted"] += int((neg0 & cnt).sum())
            seen["neg0_filtered"] += int((neg0 & (code & 0x80 != 0)).sum())
            seen["padded_rows"] += int(abn.packed_row_stride(n) < stride or n % 256 != 0)
            seen["edge"] += int(np.isin(lines % 64, (0, 63)).sum() + (lines % 3 == 0).sum())
            seen["adjacent"] += int((np.diff(lines) == 1).sum())
    assert all(v > 20 for v in seen.values()), seen


def test_hand_case(abn, L):
    """records on lines 1, 2, 5, 6, inserted lines 3, 4, 7 and no site on line 8, chunks of 3 lines: the merged bytes, the
    first dword and the fold spelled out"""
    kind = np.array([NOTHING, RECORD, RECORD, ACCEPTED, ACCEPTED, RECORD, RECORD, ACCEPTED, REJECTED])
    f = {"status": np.array([0, 2, 1, 2, 1, 0, 2, 0, 0], dtype=np.uint8),
         "pm": np.array([0.5, 0.995, 0.5, np.nan, 0.1, 0.99, 0.98, 1.0, 0.0]),
         "ml": np.array([9.0, 0.25, 8.0, 7.0, 6.0, -0.0, 5.0, 0.5, 4.0])}
    code, level, row, s, k = run(L, kind, f, 3, 64)
    assert code.tolist() == [0x42, 0x81, 0x02, 0x81, 0x40, 0x82, 0x40]           # the NaN on line 3: neither 0x80 nor 0x40
    fields = [2, 3, 2, 3, 0, 3, 0] + [3] * 9
    want = sum(v << (8 * (i & 3) + 2 * (i >> 2)) for i, v in enumerate(fields))
    assert int.from_bytes(row[:4].tobytes(), "little") == want and set(row[4:].tolist()) == {0xff}
    assert (s, k) == (struct.pack("<d", 0.25 + -0.0 + 0.5), 3)
    # a NaN level of a counted site: a NaN sum (which NaN is not pinned)
    f["ml"][1] = np.nan
    _, _, _, s, k = run(L, kind, f, 3, 64)
    assert np.isnan(struct.unpack("<d", s)[0]) and k == 3
    # ... of an uncounted one: no part of the sum
    f["ml"][1], f["ml"][2] = 0.25, np.nan
    _, _, _, s, k = run(L, kind, f, 3, 64)
    assert (s, k) == (struct.pack("<d", 0.75), 3)
    # a sum that stays +0.0 over counted -0.0 levels and uncounted sites alike
    f["ml"][:] = -0.0
    _, _, _, s, k = run(L, kind, f, 3, 64)
    assert (s, k) == (struct.pack("<d", 0.0), 3)
    t = L.abh_codes_build_serial.argtypes
    one = np.zeros(1, dtype=np.int64)
    args = lambda lines, stride: [1, one.ctypes.data_as(t[1]), np.array([4], dtype=np.int64).ctypes.data_as(t[2]), 0] + \
        [None] * 4 + [len(lines), np.array(lines, dtype=np.int64).ctypes.data_as(t[9])] + [None] * 3 + [K.FILTER, stride] + [None] * 5
    assert L.abh_codes_build_serial(*args([4], 64)) == -1                         # a line in no chunk's slab
    assert L.abh_codes_build_serial(*args([2, 2], 64)) == -1                      # lines that do not ascend
    assert L.abh_codes_build_serial(*args([], 6)) == -2                           # a row stride that is no multiple of 4


def test_build_under_address_and_ub_sanitizers(tmp_path):
    """A stand-alone program (its own main, run directly): the serial build over seeded samples of the same site counts and
    patterns at the same chunk lengths, every array in a heap block of exactly its length, against a merge by line number, a
    field-by-field pack and a plain fold written out there, built with -fsanitize=address,undefined."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.fail("g++ is needed for the sanitizer build of tests/native/codes_main.cpp")
    root = Path(__file__).resolve().parent.parent
    exe = tmp_path / "codes_main"
    r = subprocess.run([gxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                        "-fno-omit-frame-pointer", "-o", str(exe), str(root / "tests" / "native" / "codes_main.cpp")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600,
                       env={"UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1", "ASAN_OPTIONS": "abort_on_error=1"})
    assert r.returncode == 0 and "sanitized codes build ok" in r.stdout, r.stdout[-1500:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
