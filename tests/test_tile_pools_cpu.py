"""Region pools without a device: the serial forms of alphabeta_rs_amd/csrc/abn_tiles.hpp's pools (the merge of a pool's
intervals into segments, the 64-bit offsets, the map from pooled to source columns, the gather) through the host shim against
the mask model of tests/_tile_pools_model.py on the inputs the device tests use; the merge rules case by case; the name-aware
region reader and the pool numbering of host/tiles.hpp; the size limit of a pooled matrix; and the stand-alone driver
tests/native/tile_pools_main.cpp, plain and under AddressSanitizer + UndefinedBehaviorSanitizer."""
import ctypes as C
import shutil
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

import _tile_pools_model as PM
import _tiles_model as T
import _windows_model as M

ROOT = Path(__file__).resolve().parent.parent
ALIGNS = ("none", "position", "union")
N = 4
NAN_SITE = 700


@pytest.fixture(scope="module")
def L():
    L = M.hostlib()
    ll, i32p, u32p, u8p, dp = C.c_longlong, C.POINTER(C.c_int), C.POINTER(C.c_uint32), C.POINTER(C.c_uint8), C.POINTER(C.c_double)
    llp = C.POINTER(ll)
    L.abh_tiles_runs_serial.argtypes = [ll, i32p, u32p, u32p, u8p, llp, llp, i32p, llp, llp, u32p, llp, C.c_char_p, ll]
    L.abh_tiles_search_serial.argtypes = [u32p, llp, llp, ll, i32p, llp, llp, llp, llp]
    L.abh_tiles_search_serial.restype = None
    L.abh_tiles_fold_serial.argtypes = [u8p, ll, dp, ll, C.c_int, ll, llp, llp, dp, llp]
    L.abh_tiles_fold_serial.restype = None
    L.abh_tiles_pool_merge.argtypes = [C.c_int, i32p, ll, i32p, llp, llp, i32p, C.c_int, ll, i32p, i32p, llp, llp, llp]
    L.abh_tiles_pool_merge.restype = ll
    L.abh_tiles_pool_offsets_map.argtypes = [ll, llp, llp, llp, ll, llp, llp, llp, llp]
    L.abh_tiles_pool_offsets_map.restype = None
    L.abh_tiles_pool_gather_serial.argtypes = [u8p, ll, dp, ll, C.c_int, llp, ll, u8p, ll, dp]
    L.abh_tiles_pool_gather_serial.restype = None
    L.abh_tiles_matrix_fits.argtypes = [C.c_int, ll]
    L.abh_tiles_region_pools.argtypes = [C.c_char_p, ll, ll, i32p, llp, llp, i32p, llp, C.c_char_p, ll]
    L.abh_tiles_region_pools.restype = ll
    return L


def ptr(a, t):
    return a.ctypes.data_as(t)


def serial_runs(L, chrom, start, strand):
    """abh_tiles_runs_serial -> (run_begin, run_end, the runs' chromosomes in run order)"""
    n = len(chrom)
    chrom, start = np.ascontiguousarray(chrom, dtype=np.int32), np.ascontiguousarray(start, dtype=np.uint32)
    strand = np.ascontiguousarray(strand, dtype=np.uint8)
    rb, re = np.zeros(258, dtype=np.int64), np.zeros(258, dtype=np.int64)
    rc, rl = np.zeros(258, dtype=np.int32), np.zeros(258, dtype=np.uint32)
    rf, rn, refusal = np.zeros(258, dtype=np.int64), np.zeros(258, dtype=np.int64), np.zeros(3, dtype=np.int64)
    text = C.create_string_buffer(256)
    t = L.abh_tiles_runs_serial.argtypes
    k = L.abh_tiles_runs_serial(n, ptr(chrom, t[1]), ptr(start, t[2]), ptr(start.copy(), t[3]), ptr(strand, t[4]), ptr(rb, t[5]),
                                ptr(re, t[6]), ptr(rc, t[7]), ptr(rf, t[8]), ptr(rn, t[9]), ptr(rl, t[10]), ptr(refusal, t[11]),
                                text, len(text))
    assert k >= 0, text.value
    return rb, re, rc[:k].tolist()


def serial_merge(L, run_chromosomes, intervals, pool, n_pools):
    """abh_tiles_pool_merge -> (pool, chromosome, start, end lists, seg_first list)"""
    chrom, lo, hi = (np.ascontiguousarray(a, dtype=d) for a, d in zip(intervals, (np.int32, np.int64, np.int64)))
    ids, rc = np.ascontiguousarray(pool, dtype=np.int32), np.ascontiguousarray(run_chromosomes, dtype=np.int32)
    cap = len(chrom) + 1                                                       # (a merge never makes more segments than intervals)
    sp, sc = np.full(cap, -7, dtype=np.int32), np.full(cap, -7, dtype=np.int32)
    ss, se, first = np.full(cap, -7, dtype=np.int64), np.full(cap, -7, dtype=np.int64), np.full(n_pools + 1, -7, dtype=np.int64)
    t = L.abh_tiles_pool_merge.argtypes
    S = L.abh_tiles_pool_merge(len(rc), ptr(rc, t[1]), len(chrom), ptr(chrom, t[3]), ptr(lo, t[4]), ptr(hi, t[5]), ptr(ids, t[6]),
                               n_pools, cap, ptr(sp, t[9]), ptr(sc, t[10]), ptr(ss, t[11]), ptr(se, t[12]), ptr(first, t[13]))
    assert 0 <= S < cap
    return sp[:S].tolist(), sc[:S].tolist(), ss[:S].tolist(), se[:S].tolist(), first.tolist()


def serial_search(L, start, rb, re, tiles):
    chrom, lo, hi = (np.ascontiguousarray(a, dtype=d) for a, d in zip(tiles, (np.int32, np.int64, np.int64)))
    start = np.ascontiguousarray(start, dtype=np.uint32)
    begin, end = np.full(len(chrom), -7, dtype=np.int64), np.full(len(chrom), -7, dtype=np.int64)
    t = L.abh_tiles_search_serial.argtypes
    L.abh_tiles_search_serial(ptr(start, t[0]), ptr(rb, t[1]), ptr(re, t[2]), len(chrom), ptr(chrom, t[4]), ptr(lo, t[5]),
                              ptr(hi, t[6]), ptr(begin, t[7]), ptr(end, t[8]))
    return begin, end


def serial_offsets_map(L, col_begin, col_end, seg_first):
    """-> (seg_off, the pools' begin and end, src)"""
    S, P = len(col_begin), len(seg_first) - 1
    cb, ce = np.ascontiguousarray(col_begin, dtype=np.int64), np.ascontiguousarray(col_end, dtype=np.int64)
    first = np.ascontiguousarray(seg_first, dtype=np.int64)
    off, begin, end = np.full(S + 1, -7, dtype=np.int64), np.full(P, -7, dtype=np.int64), np.full(P, -7, dtype=np.int64)
    llp = C.POINTER(C.c_longlong)
    L.abh_tiles_pool_offsets_map(S, ptr(cb, llp), ptr(ce, llp), ptr(off, llp), P, ptr(first, llp), ptr(begin, llp), ptr(end, llp), None)
    src = np.full(int(off[S]), -7, dtype=np.int64)
    L.abh_tiles_pool_offsets_map(S, ptr(cb, llp), ptr(ce, llp), ptr(off, llp), P, None, None, None, ptr(src, llp))
    return off, begin, end, src


def test_serial_forms_equal_the_model(L):
    rows = T.master_sites()
    values = [T.sample_values(rows, 40 + s, nan_at=NAN_SITE if s == 1 else None) for s in range(N)]
    (ichrom, ilo, ihi, ipool), names, cases = PM.pool_list(rows)
    P = len(names)
    for align in ALIGNS:
        rng = np.random.default_rng(5)
        keeps = [list(range(len(rows)))] * N if align == "none" else \
            [sorted(set(range(len(rows))) - set(rng.choice(NAN_SITE - 1, size=9, replace=False).tolist())) for _ in range(N)]
        chrom, start, strand, cols = T.aligned(rows, values, keeps, align)
        rb, re, run_chrom = serial_runs(L, chrom, start, strand)
        assert run_chrom == [2, 1, 257]                                        # run order, not key order
        # the merge
        got = serial_merge(L, run_chrom, (ichrom, ilo, ihi), ipool, P)
        want = PM.segments(run_chrom, (ichrom, ilo, ihi), ipool, P)
        assert got == tuple(want)
        sp, sc, ss, se, first = got
        # the segments' columns, the offsets, the pools' ranges and the map
        cb, ce = serial_search(L, start, rb, re, (sc, ss, se))
        want_cb, want_ce = T.search(chrom, start, (sc, ss, se))
        assert cb.tolist() == want_cb.tolist() and ce.tolist() == want_ce.tolist()
        off, begin, end, src = serial_offsets_map(L, cb, ce, first)
        per_pool = PM.pool_columns(chrom, start, (ichrom, ilo, ihi), ipool, P)
        want_begin, want_end, want_src = PM.layout(per_pool)
        assert off.tolist() == np.concatenate([[0], np.cumsum(ce - cb)]).tolist()
        assert begin.tolist() == want_begin.tolist() and end.tolist() == want_end.tolist(), align
        assert src.tolist() == want_src.tolist(), align
        for p in range(P):                                                     # disjoint and ascending in column space
            assert np.all(np.diff(src[begin[p]:end[p]]) > 0)
        # the gather, and the existing fold over the pooled arrays
        ncol, stride, pooled = len(chrom), (len(chrom) + 15) // 16 * 16, len(src)
        pstride = (pooled + 15) // 16 * 16
        code, level = np.full((N, stride), 0x7f, dtype=np.uint8), np.zeros((N, ncol))
        for s, c in enumerate(cols):
            code[s, :ncol], level[s] = c["code"], c["level"]
        pcode, plevel = np.full((N, pstride), 0x55, dtype=np.uint8), np.full((N, pooled), -1.0)
        t = L.abh_tiles_pool_gather_serial.argtypes
        L.abh_tiles_pool_gather_serial(ptr(code, t[0]), stride, ptr(level, t[2]), ncol, N, ptr(src, t[5]), pooled, ptr(pcode, t[7]),
                                       pstride, ptr(plevel, t[9]))
        pcols = PM.pooled(cols, want_src)
        for s in range(N):
            assert pcode[s, :pooled].tolist() == pcols[s]["code"].tolist() and (pcode[s, pooled:] == 0x55).all()
            assert plevel[s].tobytes() == pcols[s]["level"].tobytes()
        sums, kept = np.full((N, P), -1.0), np.full((N, P), -1, dtype=np.int64)
        t = L.abh_tiles_fold_serial.argtypes
        L.abh_tiles_fold_serial(ptr(pcode, t[0]), pstride, ptr(plevel, t[2]), pooled, N, P, ptr(begin, t[6]), ptr(end, t[7]),
                                ptr(sums, t[8]), ptr(kept, t[9]))
        want_sums, want_kept = T.folds(pcols, want_begin, want_end)
        assert kept.tolist() == want_kept.tolist(), align
        assert [[struct.pack("<d", v) for v in row] for row in sums] == want_sums, align
        if align == "none":
            length = (ce - cb).tolist()
            assert {0, 1, 15, 16, 17, 63, 64, 65, 200} <= set(length), sorted(set(length))
            count = dict(zip(names, (end - begin).tolist()))
            assert count["nothing"] == 0 and count["one"] == 1 and count["lengths"] == 112 and count["wide"] == 329
            assert begin[names.index("wide")] % 64 != 0 and begin[names.index("one")] % 16 != 0
            a, b = src[begin[names.index("apart")]:end[names.index("apart")]].tolist()
            assert b - a == 300
            runs = src[begin[names.index("runs")]:end[names.index("runs")]]
            assert chrom[runs].tolist() == sorted(chrom[runs].tolist(), key=[2, 1, 257].index) and set(chrom[runs]) == {2, 1, 257}
            assert NAN_SITE in runs and start[runs[-1]] == T.LAST and 402 in runs and 403 in runs      # both strands at one start
            assert len(runs) == len(set(runs.tolist())) == 50 + 2 + 20 + 15 + 1                        # every column once
            e = names.index("empties")
            assert first[e + 1] - first[e] == PM.N_EMPTY + 2 and count["empties"] == 2
            assert length[first[e]] == 1 and length[first[e + 1] - 1] == 1 and not any(length[first[e] + 1:first[e + 1] - 1])
            shared = set(src[begin[names.index("shared")]:end[names.index("shared")]].tolist())
            assert set(range(7, 71)) <= shared and set(range(7, 71)) <= set(src[begin[1]:end[1]].tolist())   # one interval, two pools
        if align == "union":                                                   # a pool that holds placeholders
            held = src[begin[names.index("shared")]:end[names.index("shared")]]
            assert any((c["code"][held] == 0x80).any() for c in cols)


def test_merge_rules(L):
    runs = [5, 2, 257]                                                         # run order: 5 before 2

    def merge(rows, n_pools):
        c, a, b, p = zip(*rows) if rows else ((), (), (), ())
        got = serial_merge(L, runs, (c, a, b), p, n_pools)
        assert got == tuple(PM.segments(runs, (c, a, b), p, n_pools))
        return list(zip(*got[:4])), got[4]

    assert merge([(2, 10, 20, 0), (2, 15, 30, 0)], 1) == ([(0, 2, 10, 30)], [0, 1])                  # overlapping
    assert merge([(2, 10, 50, 0), (2, 20, 30, 0)], 1) == ([(0, 2, 10, 50)], [0, 1])                  # nested
    assert merge([(2, 10, 20, 0), (2, 20, 30, 0)], 1) == ([(0, 2, 10, 30)], [0, 1])                  # touching
    assert merge([(2, 10, 20, 0), (2, 21, 30, 0)], 1) == ([(0, 2, 10, 20), (0, 2, 21, 30)], [0, 2])  # one bp apart
    assert merge([(2, 40, 50, 0), (2, 10, 20, 0), (2, 45, 60, 0)], 1) == ([(0, 2, 10, 20), (0, 2, 40, 60)], [0, 2])   # out of order
    assert merge([(2, 10, 20, 0)] * 3, 1) == ([(0, 2, 10, 20)], [0, 1])                              # duplicates
    assert merge([(2, 10, 10, 0), (2, 30, 5, 0), (2, 7, 8, 0)], 1) == ([(0, 2, 7, 8)], [0, 1])       # end <= start
    assert merge([(9, 10, 20, 0), (256, 0, T.POS_END, 0)], 1) == ([], [0, 0])                        # no run
    assert merge([(2, 10, 20, 0), (2, 10, 20, 1)], 2) == ([(0, 2, 10, 20), (1, 2, 10, 20)], [0, 1, 2])   # in two pools
    assert merge([(2, 10, 20, 2)], 4) == ([(2, 2, 10, 20)], [0, 0, 0, 1, 1])                         # empty pools around one
    assert merge([(257, 1, 2, 0), (2, 1, 2, 0), (5, 1, 2, 0)], 1) == ([(0, 5, 1, 2), (0, 2, 1, 2), (0, 257, 1, 2)], [0, 3])
    assert merge([(2, 15, 25, 1), (2, 10, 20, 0), (2, 20, 30, 1)], 2) == ([(0, 2, 10, 20), (1, 2, 15, 30)], [0, 1, 2])   # pools do not merge
    assert merge([(2, 0, T.POS_END, 0), (2, T.POS_END, T.POS_END, 0)], 1) == ([(0, 2, 0, T.POS_END)], [0, 1])
    assert merge([], 3) == ([], [0, 0, 0, 0])


def test_empty_segments_in_a_row_and_the_offsets(L):
    """N_EMPTY empty segments between two of one column; and offsets beyond 2^32, which the scan keeps in 64 bits"""
    S = PM.N_EMPTY + 2
    cb, ce = np.full(S, 40, dtype=np.int64), np.full(S, 40, dtype=np.int64)
    cb[0], ce[0], cb[-1], ce[-1] = 7, 8, 90, 91
    off, begin, end, src = serial_offsets_map(L, cb, ce, [0, S])
    assert off[0] == 0 and (off[1:-1] == 1).all() and off[-1] == 2 and src.tolist() == [7, 90] and (begin[0], end[0]) == (0, 2)
    big = np.array([0, 3 << 30, 5, 9], dtype=np.int64)
    llp = C.POINTER(C.c_longlong)
    off = np.zeros(5, dtype=np.int64)
    L.abh_tiles_pool_offsets_map(4, ptr(big, llp), ptr(big + (3 << 30), llp), ptr(off, llp), 0, None, None, None, None)
    assert off.tolist() == [k * (3 << 30) for k in range(5)] and off[-1] > 1 << 32
    # the limits tiles_build applies to the handle's own matrix, applied to a pooled one
    assert L.abh_tiles_matrix_fits(4, 0) and L.abh_tiles_matrix_fits(4, 1 << 32) and L.abh_tiles_matrix_fits(8, 1 << 36)
    assert L.abh_tiles_matrix_fits(1, 256 * 0x7fffffff) and not L.abh_tiles_matrix_fits(1, 256 * 0x7fffffff + 1)   # a lane per column
    assert not L.abh_tiles_matrix_fits(65535, 1 << 36)                                                              # a lane per dword


def test_region_reader_names_and_pool_numbering(L):
    text = ("track name=classes\n"
            "chr1\t100\t200\tTE\t0\t+\n"
            "2 300 250 gene\n"                               # end < start: kept, an empty interval of its pool
            "chr1\t500\t900\n"                               # no name: skipped, and counted
            "C\t7\t9\tTE\n"
            "chrM\t0\t4294967296\tstate_7\r\n"
            "X\t1\t2\tTE\n"                                  # no chromosome: no row at all
            "1\t5\t6\tgene\textra\n"
            "3 1 2\n")
    cap = 16
    chrom, pool = np.zeros(cap, dtype=np.int32), np.zeros(cap, dtype=np.int32)
    lo, hi, counts = np.zeros(cap, dtype=np.int64), np.zeros(cap, dtype=np.int64), np.zeros(2, dtype=np.int64)
    names = C.create_string_buffer(256)
    t = L.abh_tiles_region_pools.argtypes

    def pools(bed, cap=cap):
        return L.abh_tiles_region_pools(bed.encode(), len(bed.encode()), cap, ptr(chrom, t[3]), ptr(lo, t[4]), ptr(hi, t[5]),
                                        ptr(pool, t[6]), ptr(counts, t[7]), names, len(names))

    n = pools(text)
    assert n == 5 and counts.tolist() == [3, 2]
    assert list(zip(chrom[:n].tolist(), lo[:n].tolist(), hi[:n].tolist(), pool[:n].tolist())) == [
        (1, 100, 200, 0), (2, 300, 250, 1), (257, 7, 9, 0), (256, 0, 1 << 32, 2), (1, 5, 6, 1)]
    assert names.value.decode() == "TE:2\ngene:2\nstate_7:1\n"              # numbered by first appearance; their rows
    assert pools(text, cap=2) == -1
    assert pools("1 5 6 a;b\n") == -2 and "';'" in names.value.decode() and "region 0" in names.value.decode()
    assert pools("1 5 6\n2 7 8\n") == 0 and counts.tolist() == [0, 2]
    assert pools("") == 0 and counts.tolist() == [0, 0]


@pytest.mark.parametrize("sanitize", [False, True])
def test_standalone_driver(tmp_path, sanitize):
    """tests/native/tile_pools_main.cpp, a program of its own (nothing is loaded into Python): plain, and with
    -fsanitize=address,undefined, every array in a heap block of exactly its length"""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.fail("g++ is needed for tests/native/tile_pools_main.cpp")
    exe = tmp_path / "tile_pools_main"
    flags = ["-fsanitize=address,undefined", "-fno-omit-frame-pointer"] if sanitize else []
    r = subprocess.run([gxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", *flags, "-o", str(exe),
                        str(ROOT / "tests" / "native" / "tile_pools_main.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600,
                       env={"UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1", "ASAN_OPTIONS": "abort_on_error=1"})
    assert r.returncode == 0 and "tile pools serial forms ok" in r.stdout, r.stdout[-1500:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
