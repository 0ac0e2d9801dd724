"""The law of the simulated methylomes (alphabeta_rs_amd/csrc/abn_sim.hpp, include/abneutral.h) in numpy, for
tests/test_sim_cpu.py, test_sim_gpu.py and test_sim_cli_gpu.py.  It never calls the code under test: Philox4x32-10 is
vectorised over the quads (the rounds oracle.philox computes, which test_sim_cpu.py holds it to), thresholds are Python
ints, and the pack is written out from the format's definition."""
import math

import numpy as np

TAG_SIM = 5
MAX64 = (1 << 64) - 1
SIZES = (1, 15, 16, 17, 255, 256, 257, 1023, 1024, 1025, 4095, 4097)   # the dword, the 64-byte step, a wavefront, a workgroup

# (name, parent, generation, emit): the shapes the device entry is held to
TREES = (
    ("founder alone", [-1], [3], [1]),
    ("chain", [-1, 0, 1, 2], [0, 1, 3, 4], [1, 1, 1, 1]),
    ("star", [-1, 0, 0, 0, 0], [1, 2, 2, 5, 9], [1, 1, 1, 1, 1]),
    ("parent not the previous node", [-1, 0, 0, 1, 1, 2, 2, 3], [2, 3, 3, 5, 8, 4, 9, 5], [1, 1, 1, 1, 1, 1, 1, 1]),
    ("unemitted internal nodes", [-1, 0, 0, 1, 1, 2, 2, 3], [2, 3, 3, 5, 8, 4, 9, 5], [1, 0, 0, 0, 1, 1, 1, 1]),
    ("unemitted founder and a dead leaf", [-1, 0, 0, 1, 1, 2, 2, 3, 4], [0, 3, 3, 5, 8, 4, 9, 5, 9], [0, 0, 1, 0, 1, 1, 0, 1, 0]),
    ("dt = 0", [-1, 0, 1, 1, 0], [2, 2, 2, 4, 2], [1, 1, 0, 1, 1]),
)
TREE8 = ([-1, 0, 0, 1, 1, 2, 2, 3], [2, 3, 3, 5, 8, 4, 9, 5])               # the statistics' tree: every node emitted


def philox(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 of the counters (c0[i], c1, c2, c3) under the key (k0, k1): four uint32 arrays"""
    m32 = np.uint64(0xFFFFFFFF)
    c0 = np.asarray(c0, dtype=np.uint64) & m32
    c = [c0, np.full_like(c0, c1), np.full_like(c0, c2), np.full_like(c0, c3)]
    k0, k1 = int(k0), int(k1)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c[0]
        p1 = np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & m32, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & m32]
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return [x.astype(np.uint32) for x in c]


def quad_counters(n_sites, first):
    """the quad counters k >> 2 of the sites [first, first + n_sites); first a multiple of 16"""
    assert first >= 0 and first % 16 == 0
    return np.arange(first // 4, first // 4 + (n_sites + 3) // 4, dtype=np.uint64)


def draw_words(seed, v, n_sites, first=0):
    """(H word, Lw word) of the sites [first, first + n_sites) of node v: uint32 (n_sites,) each"""
    quads = quad_counters(n_sites, first)
    key = (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    hi = np.stack(philox(quads, 0, v, TAG_SIM, *key), axis=1).reshape(-1)[:n_sites]
    lo = np.stack(philox(quads, 1, v, TAG_SIM, *key), axis=1).reshape(-1)[:n_sites]
    return hi, lo


def draws(seed, v, n_sites, first=0):
    hi, lo = draw_words(seed, v, n_sites, first)
    return (hi.astype(np.uint64) << np.uint64(32)) | lo.astype(np.uint64)


def states(seed, parent, thr, n_sites, first=0):
    """state uint8 (V, n_sites) of every node, emitted or not, at the sites [first, first + n_sites) (sites are
    independent: only the quad counter's origin moves); thr[v][s][i] are ints"""
    V = len(parent)
    out = np.zeros((V, n_sites), dtype=np.uint8)
    for v in range(V):
        u = draws(seed, v, n_sites, first)
        s = np.zeros(n_sites, dtype=np.intp) if v == 0 else out[parent[v]].astype(np.intp)
        t0 = np.array([int(thr[v][k][0]) for k in range(3)], dtype=np.uint64)[s]
        t1 = np.array([int(thr[v][k][1]) for k in range(3)], dtype=np.uint64)[s]
        out[v] = (u >= t0).astype(np.uint8) + (u >= t1).astype(np.uint8)
    return out


def row_stride(n_sites):
    return 0 if n_sites <= 0 else (n_sites + 255) // 256 * 64


def pack(fields, stride=None, fill=0xFF):
    """fields uint8 (rows, L) of 0..3 -> packed (rows, stride): site 16 g + 4 j + e in byte 4 g + e at bits 2j..2j+1, every
    field behind L up to row_stride(L) 3; bytes of a longer stride hold `fill`"""
    rows, L = fields.shape
    least = row_stride(L)
    stride = least if stride is None else stride
    padded = np.full((rows, 4 * least), 3, dtype=np.uint8)
    padded[:, :L] = fields
    f = padded.reshape(rows, least // 4, 4, 4).astype(np.uint32)             # [row][g][j][e]
    by = sum(f[:, :, j, :] << (2 * j) for j in range(4)).astype(np.uint8)    # [row][g][e]
    out = np.full((rows, stride), fill, dtype=np.uint8)
    out[:, :least] = by.reshape(rows, least)
    return out


def model(seed, parent, thr, emit, n_sites, stride=None, fill=0xFF, first=0):
    """the packed rows of the emitted nodes; first > 0: the bytes from byte first / 4 on of rows of first + n_sites sites
    (the padding is the row's own where first is a multiple of 256)"""
    st = states(seed, parent, thr, n_sites, first)
    return pack(st[np.flatnonzero(np.asarray(emit))], stride, fill)


def threshold(c):
    if not c > 0.0:
        return 0
    if c >= 1.0:
        return MAX64
    return int(math.ldexp(c, 64))


def thresholds_of_row(p):
    """[t0, t1] of a probability row: c0 = p[0], c1 = p[0] + p[1] with one rounded add"""
    return [threshold(float(p[0])), threshold(float(p[0]) + float(p[1]))]


def random_thresholds(rng, V):
    """ordered pairs over the whole 64-bit range, as Python ints [V][3][2]"""
    t = rng.integers(0, 1 << 64, size=(V, 3, 2), dtype=np.uint64)
    t.sort(axis=2)
    return [[[int(x) for x in pair] for pair in node] for node in t]


def as_array(thr):
    return np.array(thr, dtype=np.uint64).reshape(-1, 3, 2)


def common_generation(parent, generation, a, b):
    while a != b:
        if a > b:
            a = parent[a]
        else:
            b = parent[b]
    return generation[a]


def pedigree(st, parent, generation, emit):
    """(rows [t0, t1, t2, D], p0uu, diff, both) of the states (V, L): DMatrix::from and convert (src/pedigree.rs:210-333) on
    the emitted nodes in node order, no site filtered; p0uu from the levels state / 2 (:171-183)"""
    sampled = [v for v in range(len(parent)) if emit[v]]
    L = st.shape[1]
    rows, diff, both = [], [], []
    for a, i in enumerate(sampled):
        for j in sampled[a + 1:]:
            d = int(np.abs(st[i].astype(np.int64) - st[j].astype(np.int64)).sum())
            diff.append(d), both.append(L)
            rows.append([float(common_generation(parent, generation, i, j)), float(generation[i]), float(generation[j]),
                         d / (2.0 * float(L))])
    total = 0.0
    for v in sampled:
        n1, n2 = int((st[v] == 1).sum()), int((st[v] == 2).sum())
        total += 1.0 - float(n1 + 2 * n2) / (2.0 * float(L))
    return np.array(rows).reshape(-1, 4), total / float(len(sampled)), diff, both


def breadth_first(nodes, edges):
    """nodes [(name, generation, meth)], edges [(from, to)] in file order -> (parent, generation, emit) numbered
    breadth-first from the root, children in the edges' order"""
    names = [n[0] for n in nodes]
    children = {n: [] for n in names}
    has_parent = set()
    for a, b in edges:
        children[a].append(b)
        has_parent.add(b)
    (root,) = [n for n in names if n not in has_parent]
    order, parent = [root], [-1]
    at = 0
    while at < len(order):
        for c in children[order[at]]:
            order.append(c)
            parent.append(at)
        at += 1
    info = {n[0]: n for n in nodes}
    return parent, [info[n][1] for n in order], [1 if info[n][2] else 0 for n in order]


def planted(seed, which, delta, state, L=64, at=37):
    """(thr of the chain founder -> child, the child's state wanted at site `at`): the founder is `state` everywhere; the
    child's threshold `which` under that state is the draw at `at` plus delta in the low word"""
    hi, lo = draw_words(seed, 1, L)
    assert 0 < int(lo[at]) < 0xFFFFFFFF
    t = (int(hi[at]) << 32) | (int(lo[at]) + delta)
    founder = [(MAX64, MAX64), (0, MAX64), (0, 0)][state]
    child = [[0, MAX64]] * 3
    child[state] = [t, MAX64] if which == 0 else [0, t]
    # u >= t for delta <= 0: above the first threshold (state 1), above both (state 2)
    return [[list(founder)] * 3, child], (1 if delta <= 0 else 0) if which == 0 else (2 if delta <= 0 else 1)
