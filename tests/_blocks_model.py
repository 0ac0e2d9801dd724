"""A model of the block bootstrap (alphabeta_rs_amd/csrc/abn_blocks.hpp) that shares no code with it: the counts from the
oracle's Philox with the stated counter layout, the sums as integer products (int64: every sum stays below 2^63 inside the
limits), dvalue by the stated expression, the level sums as a serial Python loop of products and adds."""
import re
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "alphabeta_rs_amd" / "csrc" / "abn_blocks.hpp"
TAG_BLOCK = 4
IDENTITY_ID = (1 << 20) - 1
INVALID = 1  # ABN_ERR_INVALID_ARG


def constants():
    """the header's constants by name -> int"""
    text = HEADER.read_text()
    found = {}
    for name, value in re.findall(r"constexpr (?:int|long long) (kBlock\w+) = ([^;]+);", text):
        found[name] = int(eval(value.replace("LL", "").replace("1 <<", "1<<"), {"__builtins__": {}}))
    return found


def counts(oracle, seed, group_id, group_begin, group_end, n_replicates, n_blocks):
    """uint8 (G, R + 1, T): row r of group g = the histogram of T_g draws, draw j = gb + ((word * T_g) >> 32) with word =
    element j % 4 of philox(j // 4, r, group_id, 4; seed_lo, seed_hi); row R all ones; zero outside the range"""
    key = (seed & 0xffffffff, seed >> 32)
    G = len(group_begin)
    out = np.zeros((G, n_replicates + 1, n_blocks), dtype=np.int64)
    for g in range(G):
        b, Tg = int(group_begin[g]), int(group_end[g] - group_begin[g])
        out[g, n_replicates, b:b + Tg] = 1
        for r in range(n_replicates):
            for q in range((Tg + 3) // 4):
                words = oracle.philox((q, r, int(group_id[g]), TAG_BLOCK), key)
                for e in range(min(4, Tg - 4 * q)):
                    out[g, r, b + ((int(words[e]) * Tg) >> 32)] += 1
    assert out.max(initial=0) <= 127
    return out.astype(np.uint8)


def resample(group_begin, group_end, counts_u8, both, diff, level_sum_kept, kept):
    """{both, diff, dvalue: (G, rows, P); level, kept: (G, rows, n)} of explicit counts"""
    G, rows, T = counts_u8.shape
    P, n = both.shape[1], level_sum_kept.shape[0]
    c = counts_u8.astype(np.int64)
    tb, td, tk = both.astype(np.int64), diff.astype(np.int64), np.asarray(kept, dtype=np.int64)
    out = {"both": np.zeros((G, rows, P), dtype=np.uint64), "diff": np.zeros((G, rows, P), dtype=np.uint64),
           "dvalue": np.zeros((G, rows, P)), "level": np.zeros((G, rows, n)), "kept": np.zeros((G, rows, n), dtype=np.int64)}
    for g in range(G):
        b, e = int(group_begin[g]), int(group_end[g])
        out["both"][g] = (c[g, :, b:e] @ tb[b:e]).astype(np.uint64)
        out["diff"][g] = (c[g, :, b:e] @ td[b:e]).astype(np.uint64)
        out["kept"][g] = c[g, :, b:e] @ tk[:, b:e].T
        for r in range(rows):
            for s in range(n):
                acc = 0.0
                for t in range(b, e):
                    acc = acc + float(c[g, r, t]) * float(level_sum_kept[s, t])
                out["level"][g, r, s] = acc
    with np.errstate(divide="ignore", invalid="ignore"):
        out["dvalue"] = out["diff"].astype(np.float64) / (2.0 * out["both"].astype(np.float64))
    return out


def assert_equal(got, want):
    """bit for bit, NaN in the same places"""
    assert set(got) == set(want)
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        assert got[k].tobytes() == want[k].tobytes(), k


def tables(rng, T, P, n, values):
    """both / diff (T, P) drawn from `values` (every one planted at least once where they fit), levels and kept (n, T)"""
    values = np.asarray(values, dtype=np.uint64)
    both, diff = rng.choice(values, size=(T, P)), rng.choice(values, size=(T, P))
    flat_b, flat_d = both.reshape(-1), diff.reshape(-1)
    k = min(len(values), flat_b.size)
    flat_b[:k], flat_d[flat_d.size - k:] = values[:k], values[:k]
    lsk = rng.random((n, T)) * rng.integers(0, 5000, size=(n, T))
    kept = rng.integers(0, 1 << 20, size=(n, T)).astype(np.int64)
    return both, diff, lsk, kept


def planted_counts(rng, G, rows, T):
    """uint8 (G, rows, T): mostly small counts, with 0, 1 and 127 planted in every row where they fit"""
    c = rng.integers(0, 4, size=(G, rows, T)).astype(np.uint8)
    c[rng.random((G, rows, T)) < 0.1] = 127
    if T >= 3:
        c[:, :, 0], c[:, :, T // 2], c[:, :, T - 1] = 127, 0, 1
    return c


VALUES = [0, 127, 128, (1 << 14) - 1, 1 << 14, (1 << 35) - 1]


def product_cases():
    """(name, group_begin, group_end, rows, T, P, n): one group that begins and ends off a multiple of 64 for every
    combination of rows, blocks and pairs, and three groups of which one holds a single block and one is empty"""
    cases = []
    for rows in (1, 16, 17):
        for blocks in (1, 63, 64, 65, 129):
            for pairs in (1, 3, 45):
                cases.append((f"rows{rows}-blocks{blocks}-pairs{pairs}", [3], [3 + blocks], rows, blocks + 7, pairs, 2))
    cases.append(("three-groups", [5, 70, 77], [6, 70, 227], 17, 300, 45, 4))
    cases.append(("three-groups-one-pair", [63, 64, 130], [64, 64, 257], 1, 257, 1, 1))
    return cases


def product_inputs(case):
    name, gb, ge, rows, T, P, n = case
    rng = np.random.default_rng(100003 * rows + 1009 * T + P)
    gb, ge = np.array(gb, dtype=np.int64), np.array(ge, dtype=np.int64)
    return (gb, ge, planted_counts(rng, len(gb), rows, T)) + tables(rng, T, P, n, VALUES)


def flush_inputs(flush):
    """one group of flush + 65 blocks, every count 127 and every digit 127, one pair, one row"""
    T = flush + 65
    gb, ge = np.array([0], dtype=np.int64), np.array([T], dtype=np.int64)
    counts_u8 = np.full((1, 1, T), 127, dtype=np.uint8)
    both = np.full((T, 1), (1 << 35) - 1, dtype=np.uint64)
    return gb, ge, counts_u8, both, both.copy(), np.full((1, T), 0.5), np.full((1, T), 3, dtype=np.int64)


def count_group_sizes(hist):
    return [1, 3, 4, 5, 257, hist - 1, hist, hist + 1]
