"""The observation law, its thresholds, the state census and the replicate study (alphabeta_rs_amd/csrc/abn_sim.hpp,
abn_packed_census.hpp, include/abneutral.h) in numpy, for tests/test_sim_study_cpu.py, test_sim_study_gpu.py and
test_sim_study_cli_gpu.py.  Philox and the pack are _sim_model's; everything else is restated here from the law's text.
It never calls the code under test."""
import numpy as np

import _sim_model as M

TAG_OBS = 6


def obs_draw_words(seed, v, n_sites, first=0):
    """(H word, Lw word) of the observation draw of the sites [first, first + n_sites) of node v: the simulation's draw
    with c3 = 6"""
    quads = M.quad_counters(n_sites, first)
    key = (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    hi = np.stack(M.philox(quads, 0, v, TAG_OBS, *key), axis=1).reshape(-1)[:n_sites]
    lo = np.stack(M.philox(quads, 1, v, TAG_OBS, *key), axis=1).reshape(-1)[:n_sites]
    return hi, lo


def obs_draws(seed, v, n_sites, first=0):
    hi, lo = obs_draw_words(seed, v, n_sites, first)
    return (hi.astype(np.uint64) << np.uint64(32)) | lo.astype(np.uint64)


def observe_fields(seed, fields, nodes, othr, first=0):
    """fields uint8 (rows, L) of 0..3, row r the sites [first, first + L) of the methylome of node nodes[r]; othr[s][i]
    ints -> the observed fields"""
    out = np.empty_like(fields)
    L = fields.shape[1]
    for r, v in enumerate(nodes):
        w = obs_draws(seed, int(v), L, first)
        s = np.minimum(fields[r], 2).astype(np.intp)
        seen = np.zeros(L, dtype=np.uint8)
        for i in range(3):
            t = np.array([int(othr[k][i]) for k in range(3)], dtype=np.uint64)[s]
            seen += (w >= t).astype(np.uint8)
        out[r] = np.where(fields[r] == 3, 3, seen)
    return out


def unpack(packed, L):
    """packed (rows, stride) -> fields (rows, L): site 16 g + 4 j + e in byte 4 g + e at bits 2j..2j+1"""
    rows = packed.shape[0]
    least = M.row_stride(L)
    by = packed[:, :least].reshape(rows, least // 4, 1, 4)                      # [row][g][.][e]
    f = (by >> (2 * np.arange(4, dtype=np.uint8)).reshape(1, 1, 4, 1)) & 3       # [row][g][j][e]
    return f.reshape(rows, 4 * least)[:, :L].astype(np.uint8)


def observe(seed, packed, nodes, othr, L, stride=None, fill=0, first=0):
    """the observed packed matrix of a packed one: the fields behind L are 3, bytes of a longer stride hold `fill`; first > 0:
    packed holds the L sites from site `first` on of longer rows"""
    return M.pack(observe_fields(seed, unpack(packed, L), nodes, othr, first), stride, fill)


def obs_thresholds(miscall, dropout):
    """othr [3][3] as ints: c0 = q m0, c1 = q (m0 + m1), c2 = q with q = 1 - dropout, each through threshold, made
    non-decreasing"""
    out = []
    for s in range(3):
        m0, m1 = float(miscall[s][0]), float(miscall[s][1])
        q = 1.0 - float(dropout[s])
        t0, t1, t2 = M.threshold(q * m0), M.threshold(q * (m0 + m1)), M.threshold(q)
        t1 = max(t1, t0)
        out.append([t0, t1, max(t2, t1)])
    return out


def noise(e, f):
    """(miscall, dropout) of one miscall probability split over the two other states and one dropout probability"""
    m = [[1.0 - e if i == j else 0.5 * e for j in range(3)] for i in range(3)]
    return m, [f, f, f]


def census(fields, begin, end):
    """counts uint64 (windows, rows, 3) of the fields 0, 1, 2 inside [begin[w], end[w])"""
    out = np.zeros((len(begin), fields.shape[0], 3), dtype=np.uint64)
    for w, (b, e) in enumerate(zip(begin, end)):
        for f in range(3):
            out[w, :, f] = (fields[:, b:e] == f).sum(axis=1)
    return out


def random_othr(rng):
    t = rng.integers(0, 1 << 64, size=(3, 3), dtype=np.uint64)
    t.sort(axis=1)
    return [[int(x) for x in row] for row in t]


def as_array(othr):
    return np.array(othr, dtype=np.uint64).reshape(3, 3)


def study(seed, parent, generation, emit, thr, othr, L, R):
    """(times (pairs, 3), D (R, pairs), p0uu (R,), census (R, emitted, 3), both (R, pairs), observed fields (emitted, R L)) of R
    replicates as the column ranges of one simulation of R L sites; othr None: no observation step"""
    sampled = [v for v in range(len(parent)) if emit[v]]
    fields = M.states(seed, parent, thr, R * L)[sampled]
    if othr is not None:
        fields = observe_fields(seed, fields, sampled, othr)
    n = len(sampled)
    times = np.array([[float(M.common_generation(parent, generation, i, j)), float(generation[i]), float(generation[j])]
                      for a, i in enumerate(sampled) for j in sampled[a + 1:]]).reshape(-1, 3)
    counts = census(fields, [r * L for r in range(R)], [(r + 1) * L for r in range(R)])
    D, both, p0uu = np.zeros((R, n * (n - 1) // 2)), np.zeros((R, n * (n - 1) // 2), dtype=np.int64), np.zeros(R)
    for r in range(R):
        f = fields[:, r * L:(r + 1) * L].astype(np.int64)
        p = 0
        for a in range(n):
            for b in range(a + 1, n):
                kept = (f[a] < 3) & (f[b] < 3)
                d, c = int(np.abs(f[a] - f[b])[kept].sum()), int(kept.sum())
                both[r, p] = c
                D[r, p] = float(d) / (2.0 * float(c)) if c else float("nan")
                p += 1
        total = 0.0
        for s in range(n):
            n0, n1, n2 = (int(x) for x in counts[r, s])
            kept = n0 + n1 + n2
            total += 1.0 - (float(n1 + 2 * n2) / (2.0 * float(kept)) if kept else float("nan"))
        p0uu[r] = total / float(n)
    return times, D, p0uu, counts, both, fields
