"""A numpy model of region-level states (alphabeta_rs_amd/csrc/abn_regions.hpp): unpacks, counts and calls with Python
integers, builds the output through _sim_model.pack, and never calls the code under test.

The law: for sample s and window [b, e) let n0, n1, n2 be the fields 0, 1, 2 inside it, kept = n0 + n1 + n2, m = n1 + 2 n2;
the region's field is 3 if kept < min_kept, 0 if m den < lo 2 kept, 2 if m den > hi 2 kept, else 1."""
import numpy as np

import _sim_model as S


def unpack(packed, n_sites):
    """packed (rows, stride) uint8 -> fields uint8 (rows, n_sites)"""
    packed = np.asarray(packed, dtype=np.uint8)
    rows = packed.shape[0]
    k = np.arange(n_sites)
    if n_sites == 0:
        return np.zeros((rows, 0), dtype=np.uint8)
    return ((packed[:, (k >> 4) * 4 + (k & 3)] >> (2 * ((k >> 2) & 3))) & 3).astype(np.uint8)


def call(n0, n1, n2, lo, hi, den, min_kept=1):
    n0, n1, n2, lo, hi, den = int(n0), int(n1), int(n2), int(lo), int(hi), int(den)
    kept = n0 + n1 + n2
    if kept < int(min_kept):
        return 3
    m = n1 + 2 * n2
    if m * den < lo * 2 * kept:
        return 0
    if m * den > hi * 2 * kept:
        return 2
    return 1


def counts(fields, begin, end):
    """int64 (T, rows, 3): the fields 0, 1, 2 of every row inside every window, from prefix sums"""
    fields = np.asarray(fields)
    rows, L = fields.shape
    b, e = np.asarray(begin, dtype=np.int64), np.asarray(end, dtype=np.int64)
    out = np.zeros((len(b), rows, 3), dtype=np.int64)
    for f in range(3):
        pre = np.zeros((rows, L + 1), dtype=np.int64)
        np.cumsum(fields == f, axis=1, out=pre[:, 1:])
        out[:, :, f] = (pre[:, e] - pre[:, b]).T
    return out


def region_fields(fields, begin, end, rule, src=None):
    """uint8 (rows, C): the called field of window src[c] (None: the identity) of every row"""
    lo, hi, den, min_kept = rule
    cnt = counts(fields, begin, end)
    T, rows, _ = cnt.shape
    called = np.array([[call(*cnt[t, s].tolist(), lo, hi, den, min_kept) for t in range(T)] for s in range(rows)],
                      dtype=np.uint8).reshape(rows, T)
    return called if src is None else called[:, np.asarray(src, dtype=np.int64)]


def region_states(packed, n_sites, begin, end, rule, src=None):
    """the packed region matrix (rows, row_stride(C))"""
    return S.pack(region_fields(unpack(packed, n_sites), begin, end, rule, src))


def random_fields(rng, rows, L, p=(0.35, 0.2, 0.3, 0.15)):
    return rng.choice(4, size=(rows, L), p=p).astype(np.uint8)


def group_order(group, n_groups):
    """(src int32 (C,), group_begin, group_end int64 (G,)): the tiles in ascending (group, tile), -1 left out"""
    group = np.asarray(group, dtype=np.int64)
    src = [t for g in range(n_groups) for t in np.flatnonzero(group == g).tolist()]
    sizes = [int((group == g).sum()) for g in range(n_groups)]
    gb = np.concatenate(([0], np.cumsum(sizes)[:-1])).astype(np.int64)
    return np.array(src, dtype=np.int32), gb, gb + np.array(sizes, dtype=np.int64)


def pair_tables(fields, begin, end):
    """uint64 (W, pairs, 3, 3): the joint states of every pair a < b inside every window, the sites both keep"""
    fields = np.asarray(fields)
    n = fields.shape[0]
    pairs = [(a, b) for a in range(n) for b in range(a + 1, n)]
    out = np.zeros((len(begin), len(pairs), 3, 3), dtype=np.uint64)
    for w, (b0, e0) in enumerate(zip(begin, end)):
        for p, (a, b) in enumerate(pairs):
            x, y = fields[a, b0:e0], fields[b, b0:e0]
            keep = (x < 3) & (y < 3)
            np.add.at(out[w, p], (x[keep], y[keep]), 1)
    return out


def pairwise(fields, begin, end):
    """(diff uint64, both uint64, dvalue), each (W, pairs), from the pair tables: diff = sum |x - y| table, dvalue = diff / (2 both)"""
    t = pair_tables(fields, begin, end).astype(np.int64)
    w = np.abs(np.arange(3)[:, None] - np.arange(3)[None, :])
    diff, both = (t * w).sum(axis=(2, 3)), t.sum(axis=(2, 3))
    with np.errstate(invalid="ignore", divide="ignore"):
        dval = diff.astype(np.float64) / (2.0 * both.astype(np.float64))
    return diff.astype(np.uint64), both.astype(np.uint64), dval
