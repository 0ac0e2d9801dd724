"""What the tests of the collapse of repeated sites share (tests/test_sites_dedup_cpu.py, tests/test_sites_dedup_gpu.py): a
numpy / pure-Python model that never calls the code under test — run ids from cumsum(key != previous key), first and last
by np.unique, DROP by run counts, BEST by a plain Python loop per run — the host shims of host_capi.cpp, and the case
generators: key patterns in canonical order with repeats, posteriors with NaN, signed zeros and exact ties, and doubled
methylome texts."""
import ctypes as C
import math

import numpy as np

import _parse_model as P

POLICIES = ("first", "last", "best", "drop")
TILE = 2048
SIZES = (0, 1, 2, 63, 64, 65, TILE - 1, TILE, TILE + 1, 3 * TILE + 17)
LONG_RUN = 2 * TILE + 5


def hostlib():
    L = P.hostlib()
    ll, vp = C.c_longlong, C.c_void_p
    L.abn_sites_dedup_keys_host.argtypes = [ll, vp, vp, vp, vp, vp, vp, C.c_int, vp, vp, vp]
    L.abh_sites_dedup_walk.argtypes = [ll, vp, vp, vp, vp, vp, vp, C.c_int, ll, vp, vp, vp]
    return L


def records(chromosome, start, end, strand, posteriormax, status):
    return (np.ascontiguousarray(chromosome, dtype=np.int32), np.ascontiguousarray(start, dtype=np.uint32),
            np.ascontiguousarray(end, dtype=np.uint32), np.ascontiguousarray(strand, dtype=np.uint8),
            np.ascontiguousarray(posteriormax, dtype=np.float64), np.ascontiguousarray(status, dtype=np.uint8))


def better(new: float, best: float) -> bool:
    """the rule of include/abneutral.h, ABN_DEDUP_BEST"""
    return new > best or (math.isnan(best) and not math.isnan(new))


def run_ids(r):
    """the run every record belongs to, and whether a record's key equals its predecessor's"""
    n = len(r[0])
    same = np.ones(max(n - 1, 0), dtype=bool)
    for a in r[:4]:
        same &= a[1:] == a[:-1]
    ids = np.zeros(n, dtype=np.int64)
    if n > 1:
        ids[1:] = np.cumsum(~same)
    return ids, same


def first_descent(r) -> int:
    """the first record whose key lies below its predecessor's in canonical order; -1: none"""
    cols = [a.astype(np.int64) for a in r[:4]]
    below = np.zeros(max(len(cols[0]) - 1, 0), dtype=bool)
    same = np.ones_like(below)
    for a in cols:
        below |= same & (a[1:] < a[:-1])
        same &= a[1:] == a[:-1]
    hit = np.flatnonzero(below)
    return int(hit[0]) + 1 if hit.size else -1


def model(r, policy):
    """(order int64 ascending, [sites, kept, repeated keys, disagreeing neighbours]) of records without a descent"""
    n = len(r[0])
    ids, same = run_ids(r)
    if n == 0:
        return np.zeros(0, dtype=np.int64), [0, 0, 0, 0]
    _, first, counts = np.unique(ids, return_index=True, return_counts=True)
    _, rlast = np.unique(ids[::-1], return_index=True)
    last = n - 1 - rlast
    if policy == "first":
        order = first
    elif policy == "last":
        order = last
    elif policy == "drop":
        order = first[counts == 1]
    elif policy == "best":
        pm = r[4].tolist()
        order = []
        for lo, hi in zip(first.tolist(), last.tolist()):
            best = lo
            for j in range(lo + 1, hi + 1):
                if better(pm[j], pm[best]):
                    best = j
            order.append(best)
    else:
        raise ValueError(policy)
    order = np.asarray(order, dtype=np.int64)
    disagreeing = int((same & (r[5][1:] != r[5][:-1])).sum())
    return order, [n, int(order.shape[0]), int((counts > 1).sum()), disagreeing]


PM_VALUES = np.array([np.nan, -0.0, 0.0, 0.5, 0.5, 0.75, 0.99, 0.99, 1.0])


def from_runs(lengths, seed, all_nan_every=0):
    """records in canonical order whose runs have these lengths: distinct ascending keys over three chromosomes (0, 256,
    257), each repeated; posteriors from PM_VALUES (NaN, -0.0, +0.0 and exact ties), statuses 0..2.  all_nan_every k > 0:
    every k-th run holds only NaN"""
    rng = np.random.default_rng(seed)
    lengths = np.asarray(lengths, dtype=np.int64)
    m = lengths.shape[0]
    i = np.arange(m, dtype=np.int64)
    chrom = np.array([0, 256, 257])[np.minimum(i * 3 // max(m, 1), 2)]
    start = 100 + 3 * (i // 2)                      # two keys per start: they differ in the strand (or the end)
    end = start + 1 + (i % 2) * (i % 3 == 0)
    strand = np.where(end == start + 1, (i % 2) * 2, 0)
    rep = lambda a: np.repeat(a, lengths)
    n = int(lengths.sum())
    pm = PM_VALUES[rng.integers(0, len(PM_VALUES), n)]
    if all_nan_every:
        ids = rep(i)
        pm = np.where(ids % all_nan_every == 0, np.nan, pm)
    return records(rep(chrom), rep(start), rep(end), rep(strand), pm, rng.integers(0, 3, n))


def fit(lengths, n):
    """the run lengths cut or padded with single records to n records in all"""
    out, total = [], 0
    for v in lengths:
        if total >= n:
            break
        v = min(int(v), n - total)
        out.append(v)
        total += v
    return out + [1] * (n - total)


def patterns(n, seed):
    """(name, records) of every pattern of n records"""
    rng = np.random.default_rng(seed)
    straddle = []
    while sum(straddle) < n:                         # a run of two begins at records 63, 127, 191, ..
        straddle += [1] * (63 if not straddle else 62) + [2]
    out = [("no repeats", from_runs([1] * n, seed)),
           ("all equal", from_runs(fit([n], n), seed + 1)),
           ("pairs", from_runs(fit([2] * (n // 2 + 1), n), seed + 2)),
           ("random runs", from_runs(fit(rng.integers(1, 6, n + 1), n), seed + 3)),
           ("all-NaN runs", from_runs(fit(rng.integers(1, 6, n + 1), n), seed + 4, all_nan_every=3)),
           ("straddling", from_runs(fit(straddle, n), seed + 5))]
    if n >= 7:
        out.append(("start and end", from_runs([3] + [1] * (n - 6) + [3], seed + 6)))
    if n > LONG_RUN + 2:
        before = (n - LONG_RUN) // 2
        out.append(("long run", from_runs([1] * before + [LONG_RUN] + [1] * (n - LONG_RUN - before), seed + 7)))
    return out


def host_dedup(L, r, policy, walk_blocks=None):
    """the serial host form, or (walk_blocks) the walk of the kernels' structure: (rc, order, info4, first descent or
    check4)"""
    n = len(r[0])
    order, info, extra = np.full(n, -1, dtype=np.int64), np.zeros(4, dtype=np.int64), np.full(4, -7, dtype=np.int64)
    ptrs = [a.ctypes.data for a in r]
    p = POLICIES.index(policy) if isinstance(policy, str) else policy
    if walk_blocks is None:
        rc = L.abn_sites_dedup_keys_host(n, *ptrs, p, order.ctypes.data, info.ctypes.data, extra.ctypes.data)
        return rc, order[:max(int(info[1]), 0)], info.tolist(), int(extra[0])
    rc = L.abh_sites_dedup_walk(n, *ptrs, p, walk_blocks, order.ctypes.data, info.ctypes.data, extra.ctypes.data)
    return rc, order[:int(info[1])], info.tolist(), extra.tolist()


# ---- methylome texts
def doubled_text(text: bytes, seed=None, skip_lines=0, subset=None):
    """(text, copies made).  The text's lines followed by a second copy of its site lines (of those at the indices
    `subset`, counted among the lines below skip_lines; None: all) whose posteriormax is halved and whose status is
    changed; with a seed, everything below the first skip_lines shuffled by it — without one every copy stands behind its
    original.  A line that does not look like a site (fewer than 9 tab-separated fields, a posteriormax that is no
    finite number, a status outside U, I, M) is not copied."""
    lines = text.split(b"\n")
    tail = lines.pop() if lines and lines[-1] == b"" else None
    head, body = lines[:skip_lines], lines[skip_lines:]
    copies = []
    for k, line in enumerate(body):
        if subset is not None and k not in subset:
            continue
        f = line.split(b"\t")
        if len(f) < 9:
            continue
        try:
            pm = float(f[6])
        except ValueError:
            continue
        if f[7] not in (b"U", b"I", b"M") or not math.isfinite(pm):
            continue
        f[6] = repr(pm / 2).encode()
        f[7] = {b"U": b"M", b"I": b"U", b"M": b"I"}[f[7]]
        copies.append(b"\t".join(f))
    both = body + copies
    perm = np.random.default_rng(seed).permutation(len(both)) if seed is not None else range(len(both))
    return b"\n".join(head + [both[i] for i in perm]) + (b"\n" if tail is not None else b""), len(copies)


def fetch_records(f):
    """the records of a Sites.fetch() dict"""
    return records(f["chromosome"], f["start"], f["end"], f["strand"], f["posteriormax"], f["status"])
