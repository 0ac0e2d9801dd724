"""Region pools (alphabeta_rs_amd/csrc/abn_tiles.hpp: pools) as a plain numpy / Python model, and the pools the pool tests
share.  A pool is a set of intervals; its columns are the columns whose (chromosome, start) lies in at least one of them, each
once, in ascending column order: per pool a boolean mask over the columns from a plain loop over the intervals, then
np.flatnonzero.  Side by side the pools' columns are the pooled matrix; the folds and the pairwise integers are
_tiles_model's over the pooled columns.  segments() restates the merge rule of the definition in the plainest way.  No
product code."""
import numpy as np

import _tiles_model as T


# ---------------------------------------------------------------- the model
def pool_columns(chromosome, start, intervals, pool, n_pools):
    """-> [per pool: the int64 indices of its columns, ascending]"""
    chromosome, start = np.asarray(chromosome), np.asarray(start, dtype=np.int64)
    chrom, lo, hi = (np.asarray(a).tolist() for a in intervals)
    out = []
    for p in range(n_pools):
        mask = np.zeros(len(chromosome), dtype=bool)
        for c, a, b, q in zip(chrom, lo, hi, np.asarray(pool).tolist()):
            if q == p:
                mask |= (chromosome == c) & (start >= a) & (start < b)
        out.append(np.flatnonzero(mask).astype(np.int64))
    return out


def layout(per_pool):
    """-> (begin, end int64 per pool in pooled column space, src int64: every pooled column's source column)"""
    length = np.array([len(c) for c in per_pool], dtype=np.int64)
    end = np.cumsum(length)
    src = np.concatenate(per_pool) if per_pool else np.zeros(0, dtype=np.int64)
    return end - length, end, src.astype(np.int64)


def pooled(columns, src):
    """aligned(...)'s samples restricted to the pooled columns"""
    return [{k: v[src] for k, v in s.items()} for s in columns]


def segments(run_chromosomes, intervals, pool, n_pools):
    """The merge: pool by pool, the chromosomes in run order (one without a run dropped), intervals with end <= start
    dropped, the rest sorted by (start, end), overlapping or touching ones joined.
    -> (pool, chromosome, start, end lists in segment order, seg_first [n_pools + 1])"""
    chrom, lo, hi = (np.asarray(a).tolist() for a in intervals)
    ids = np.asarray(pool).tolist()
    out, first = [], [0]
    for p in range(n_pools):
        for c in run_chromosomes:
            mine = sorted((a, b) for cc, a, b, q in zip(chrom, lo, hi, ids) if q == p and cc == c and b > a)
            merged = []
            for a, b in mine:
                if merged and a <= merged[-1][1]:
                    merged[-1][1] = max(merged[-1][1], b)
                else:
                    merged.append([a, b])
            out += [(p, c, a, b) for a, b in merged]
        first.append(len(out))
    return [s[0] for s in out], [s[1] for s in out], [s[2] for s in out], [s[3] for s in out], first


# ---------------------------------------------------------------- inputs
N_EMPTY = 5000            # the empty segments in a row of the pool "empties"


def pool_list(rows):
    """The pools of the tests over the sites of master_sites() -> (chromosome int32, start int64, end int64, pool int32),
    the pools' names in pool order, and per interval the name of its case.  The intervals come in no order: neither the
    pools' nor the columns'."""
    s2 = [r[1] for r in rows if r[0] == "2"]               # the start of every column of run "2" (columns 0 ..)
    s1 = [r[1] for r in rows if r[0] == "1"]
    E = T.POS_END
    cases = [
        # lengths: segments of 1, 15, 16, 17 and 63 columns and one of none (between two sites): 112 columns
        ("lengths", "63", "2", s2[60], s2[123]), ("lengths", "1", "2", s2[0], s2[0] + 1),
        ("lengths", "17", "2", s2[40], s2[57]), ("lengths", "15", "2", s2[2], s2[17]),
        ("lengths", "0", "2", s2[130] + 1, s2[131]), ("lengths", "16", "2", s2[20], s2[36]),
        # wide: 64, 65 and 200 columns, begins at pooled column 112 (no multiple of 64); holds both strands at one start
        ("wide", "200", "2", s2[150], s2[350]), ("wide", "64", "2", s2[7], s2[71]), ("wide", "65", "2", s2[80] - 3, s2[145] - 3),
        # nothing: a chromosome without a run, end <= start, behind the run -> an empty pool (at 441: no multiple of 16)
        ("nothing", "no run", "7", 0, E), ("nothing", "end = start", "2", 500, 500), ("nothing", "end < start", "2", 900, 100),
        ("nothing", "absent M", "M", 5, 50000), ("nothing", "behind", "2", s2[-1] + 1, s2[-1] + 5000),
        ("one", "one column", "2", s2[5], s2[5] + 1),
        ("apart", "a", "2", s2[310], s2[310] + 1), ("apart", "b", "2", s2[10], s2[10] + 1),      # 300 columns apart
        # runs: all three runs, listed C, 1, 2 (run order is 2, 1, C); overlapping, nested, touching, a duplicate
        ("runs", "last site", "C", T.LAST - 10, E), ("runs", "over the gap", "1", s1[90], s1[110]),
        ("runs", "nan site", "1", s1[170], s1[185]), ("runs", "both strands", "2", s2[402], s2[402] + 1),
        ("runs", "overlaps b", "2", 200, 500), ("runs", "overlaps a", "2", 100, 300), ("runs", "nested", "2", 250, 260),
        ("runs", "touches", "2", 500, 600), ("runs", "duplicate", "2", 100, 300), ("runs", "absent", "M", 5, 50000),
        # shared: an interval of "wide" once more, and the whole of run 1 (under union: placeholders)
        ("shared", "64 again", "2", s2[7], s2[71]), ("shared", "whole run 1", "1", 0, E),
    ]
    # empties: N_EMPTY intervals without a column, one bp each and one bp apart, in the gap inside chromosome 1, between two
    # segments of one column
    cases += [("empties", "right", "1", s1[103], s1[103] + 1)]
    cases += [("empties", "empty", "1", 1000 + 2 * k, 1001 + 2 * k) for k in range(N_EMPTY)][::-1]
    cases += [("empties", "left", "1", s1[98], s1[98] + 1)]
    names = ["lengths", "wide", "nothing", "one", "apart", "runs", "shared", "empties"]
    arrays = (np.array([T.chromosome_key(c[2]) for c in cases], dtype=np.int32), np.array([c[3] for c in cases], dtype=np.int64),
              np.array([c[4] for c in cases], dtype=np.int64), np.array([names.index(c[0]) for c in cases], dtype=np.int32))
    return arrays, names, [c[1] for c in cases]
