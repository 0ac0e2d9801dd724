"""The merge of the parser's device records with the host-decided lines (alphabeta_rs_amd/csrc/abn_sites_merge.hpp) in its
serial form, through the host shim: against a Python merge by line number.  The index functions and the `code` expression
the kernels run are the ones this form runs; the chunk length is a parameter here, a slab's line count on the device."""
import ctypes as C
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import _windows_model as M

FILTER = 0.99
RECORD, ACCEPTED, REJECTED, NOTHING = 0, 1, 2, 3       # a line: a device record, deferred and a site, deferred and none, no site
PATTERNS = ("none", "every_line", "chunk_edges", "adjacent", "empty_chunk", "all_deferred", "all_rejected", "mixed")
CHUNK_LINES = (1, 2, 3, 64, 0)                          # 0: the whole file is one chunk


def hostlib():
    L = M.hostlib()
    ll, u32p, u8p, dp = C.c_longlong, C.POINTER(C.c_uint32), C.POINTER(C.c_uint8), C.POINTER(C.c_double)
    llp, i32p = C.POINTER(ll), C.POINTER(C.c_int32)
    L.abh_sites_merge_serial.argtypes = [C.c_int, llp, llp, ll, u32p, u32p, u32p, u32p, dp, dp, ll, llp, i32p, u32p, u32p,
                                         u8p, u8p, dp, dp, C.c_double, i32p, u32p, u32p, u8p, u8p, dp, llp, llp]
    L.abh_sites_merge_serial.restype = C.c_int
    return L


def make_case(seed):
    """the lines 1 .. n of a file (line 0 is the header: no site) with a class each and, for the sites, their fields"""
    rng = np.random.default_rng(seed)
    pattern = PATTERNS[seed % len(PATTERNS)]
    n = int(rng.integers(1, 601))
    kind = np.where(rng.random(n + 1) < 0.7, RECORD, NOTHING)
    chunk = int(rng.choice([1, 2, 3, 64]))               # the pattern's chunk; every chunk length is run on the case
    if pattern == "every_line" or pattern == "all_deferred":
        kind[:] = ACCEPTED
    elif pattern == "all_rejected":
        kind[:] = REJECTED
    elif pattern == "chunk_edges":
        kind[::chunk] = ACCEPTED                           # the first line of every chunk of that length
        kind[chunk - 1::chunk] = np.where(rng.random(len(kind[chunk - 1::chunk])) < 0.5, ACCEPTED, REJECTED)   # the last
    elif pattern == "adjacent":
        for at in rng.integers(1, n + 1, size=3):
            kind[at:at + 2] = ACCEPTED
    elif pattern == "empty_chunk":
        c = int(rng.integers(0, n // max(chunk, 1) + 1)) * chunk
        kind[c:c + chunk] = np.where(rng.random(len(kind[c:c + chunk])) < 0.5, ACCEPTED, NOTHING)
    elif pattern == "mixed":
        kind = rng.choice([RECORD, ACCEPTED, REJECTED, NOTHING], size=n + 1, p=[.55, .2, .1, .15])
    kind[0] = NOTHING
    f = {"chromosome": rng.integers(0, 258, size=n + 1).astype(np.int32), "start": rng.integers(0, 2 ** 32, size=n + 1, dtype=np.uint64).astype(np.uint32),
         "end": rng.integers(0, 2 ** 32, size=n + 1, dtype=np.uint64).astype(np.uint32), "strand": rng.integers(0, 3, size=n + 1).astype(np.uint8),
         "status": rng.integers(0, 3, size=n + 1).astype(np.uint8), "flag": (rng.random(n + 1) < 0.05).astype(np.uint32),
         "pm": np.where(rng.random(n + 1) < 0.5, 0.99, rng.random(n + 1)), "ml": rng.random(n + 1)}
    f["pm"][(kind == ACCEPTED) & (rng.random(n + 1) < 0.3)] = np.nan   # only the host's parser yields a NaN posterior
    return pattern, kind, f


def run(L, kind, f, chunk_lines):
    n_lines = len(kind)
    chunk_lines = chunk_lines or n_lines
    rec = np.flatnonzero(kind == RECORD)
    ins = np.flatnonzero(kind == ACCEPTED).astype(np.int64)
    n_chunks = (n_lines + chunk_lines - 1) // chunk_lines
    lines = np.minimum(chunk_lines, n_lines - chunk_lines * np.arange(n_chunks)).astype(np.int64)
    count = np.bincount(rec // chunk_lines, minlength=n_chunks).astype(np.int64)
    col = lambda a, t: np.ascontiguousarray(a, dtype=t)
    meta = f["chromosome"][rec].astype(np.uint32) | f["strand"][rec].astype(np.uint32) << 16 | \
        f["status"][rec].astype(np.uint32) << 20 | f["flag"][rec] << 24
    r = [col(rec % chunk_lines, np.uint32), col(meta, np.uint32), col(f["start"][rec], np.uint32), col(f["end"][rec], np.uint32),
         col(f["pm"][rec], np.float64), col(f["ml"][rec], np.float64)]
    i = [col(ins, np.int64), col(f["chromosome"][ins], np.int32), col(f["start"][ins], np.uint32), col(f["end"][ins], np.uint32),
         col(f["strand"][ins], np.uint8), col(f["status"][ins], np.uint8), col(f["pm"][ins], np.float64), col(f["ml"][ins], np.float64)]
    total = len(rec) + len(ins)
    out = [np.full(total, -7, dtype=np.int32), np.full(total, 7, dtype=np.uint32), np.full(total, 7, dtype=np.uint32),
           np.full(total, 7, dtype=np.uint8), np.full(total, 7, dtype=np.uint8), np.full(total, -7.0)]
    dest_r, dest_i = np.full(len(rec), -1, dtype=np.int64), np.full(len(ins), -1, dtype=np.int64)
    types = L.abh_sites_merge_serial.argtypes
    p = lambda a, t: a.ctypes.data_as(t)
    rc = L.abh_sites_merge_serial(n_chunks, p(count, types[1]), p(lines, types[2]), 0, *(p(a, t) for a, t in zip(r, types[4:10])),
                                  len(ins), *(p(a, t) for a, t in zip(i, types[11:19])), FILTER,
                                  *(p(a, t) for a, t in zip(out, types[20:26])), p(dest_r, types[26]), p(dest_i, types[27]))
    assert rc == 0
    return rec, ins, out, dest_r, dest_i


def check(L, kind, f, chunk_lines, label):
    rec, ins, out, dest_r, dest_i = run(L, kind, f, chunk_lines)
    merged = np.flatnonzero((kind == RECORD) | (kind == ACCEPTED))            # the Python merge: the sites by line number
    place = {int(l): k for k, l in enumerate(merged)}
    assert dest_r.tolist() == [place[int(l)] for l in rec], label
    assert dest_i.tolist() == [place[int(l)] for l in ins], label
    assert sorted(dest_r.tolist() + dest_i.tolist()) == list(range(len(merged))), label
    want_code = np.array([M.code_of({"status": int(f["status"][l]), "posteriormax": float(f["pm"][l])}, FILTER) for l in merged],
                         dtype=np.uint8)
    assert out[4].tobytes() == want_code.tobytes(), label
    for got, key, t in zip(out[:4] + out[5:], ("chromosome", "start", "end", "strand", "ml"),
                           (np.int32, np.uint32, np.uint32, np.uint8, np.float64)):
        assert got.tobytes() == f[key][merged].astype(t).tobytes(), (label, key)
    return len(rec), len(ins), int(np.count_nonzero(kind == REJECTED))


def test_serial_merge_against_the_merge_by_line_number():
    L = hostlib()
    seen = {p: [0, 0, 0] for p in PATTERNS}
    nan_kept = 0
    for seed in range(300):
        pattern, kind, f = make_case(seed)
        for chunk_lines in CHUNK_LINES:
            n_rec, n_ins, n_rej = check(L, kind, f, chunk_lines, (seed, pattern, chunk_lines))
        for k, v in enumerate((n_rec, n_ins, n_rej)):
            seen[pattern][k] += v
        nan_kept += int(np.count_nonzero(np.isnan(f["pm"][kind == ACCEPTED])))
    assert seen["none"][1] == 0 and seen["none"][0] > 0
    assert seen["every_line"][0] == 0 and seen["every_line"][1] > 0          # a sample whose every line is deferred
    assert seen["all_rejected"][:2] == [0, 0] and seen["all_rejected"][2] > 0  # n_inserted == 0 < n_deferred
    assert all(seen[p][1] > 0 for p in ("chunk_edges", "adjacent", "empty_chunk", "mixed"))
    assert seen["mixed"][2] > 0 and seen["chunk_edges"][2] > 0                 # n_inserted < n_deferred
    assert nan_kept > 100                                                      # NaN < filter is false: code without 0x80


def test_hand_cases():
    """the places spelled out: records on lines 1, 2, 5, 6, inserted lines 3, 4, 7 and 0 sites on line 8, chunks of 3 lines"""
    L = hostlib()
    kind = np.array([NOTHING, RECORD, RECORD, ACCEPTED, ACCEPTED, RECORD, RECORD, ACCEPTED, REJECTED])
    _, _, f = make_case(1)
    f = {k: v[:len(kind)].copy() for k, v in f.items()}
    f["pm"][:] = [0.5, 0.995, 0.5, np.nan, 0.1, 0.99, 0.98, 1.0, 0.0]
    f["status"][:] = [0, 2, 1, 2, 1, 0, 2, 0, 0]
    rec, ins, out, dest_r, dest_i = run(L, kind, f, 3)
    assert dest_r.tolist() == [0, 1, 4, 5] and dest_i.tolist() == [2, 3, 6]
    assert out[4].tolist() == [2, 0x81, 2, 0x81, 0, 0x82, 0]
    check(L, kind, f, 3, "hand")
    # an inserted line in no chunk, and lines that do not ascend, are refused by the chunk choice
    types = L.abh_sites_merge_serial.argtypes
    one = np.zeros(1, dtype=np.int64)
    args = lambda lines: [1, one.ctypes.data_as(types[1]), np.array([4], dtype=np.int64).ctypes.data_as(types[2]), 0] + \
        [None] * 6 + [len(lines), np.array(lines, dtype=np.int64).ctypes.data_as(types[11])] + [None] * 7 + [FILTER] + [None] * 8
    assert L.abh_sites_merge_serial(*args([4])) == -1
    assert L.abh_sites_merge_serial(*args([2, 2])) == -1


def test_merge_under_address_and_ub_sanitizers(tmp_path):
    """A stand-alone program (its own main, run directly): the serial merge over seeded cases of the same patterns at the
    same chunk lengths, every array in a heap block of exactly its length, against a merge by line number, built with
    -fsanitize=address,undefined."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.fail("g++ is needed for the sanitizer build of tests/native/sites_merge_main.cpp")
    root = Path(__file__).resolve().parent.parent
    exe = tmp_path / "sites_merge_main"
    r = subprocess.run([gxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-o",
                        str(exe), str(root / "tests" / "native" / "sites_merge_main.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600,
                       env={"UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1", "ASAN_OPTIONS": "abort_on_error=1"})
    assert r.returncode == 0 and "sanitized sites merge ok" in r.stdout, r.stdout[-1500:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
