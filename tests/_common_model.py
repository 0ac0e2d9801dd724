"""What the tests of the common-site step share (tests/test_sites_common_cpu.py, tests/test_sites_common_gpu.py): the
definition of include/abneutral.h ("methylomes aligned by position") spelled out in Python with sets and dictionaries of
key tuples — no search, no table of runs — and the generator of samples with a known common set."""
import numpy as np

SPLIT, NOT_ASCENDING, BAD_KEY, NOT_COORDERED = 1, 2, 3, 4          # CommonRefusal.kind of csrc/abn_sites_common.hpp
WORDS = {SPLIT: "split run", NOT_ASCENDING: "not ascending", NOT_COORDERED: "not co-ordered"}


def concat(samples):
    """samples: [[(chromosome, start, end, strand)]] -> (site_offset, chromosome, start, end, strand)"""
    off = np.zeros(len(samples) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(s) for s in samples])
    flat = [k for s in samples for k in s]
    col = lambda j, t: np.array([k[j] for k in flat], dtype=t)
    return off, col(0, np.int32), col(1, np.uint32), col(2, np.uint32), col(3, np.uint8)


def model(samples):
    """-> ("ok", keep per sample, n_common) or ("refused", kind, sample, site): the lowest offending site of the whole input
    among split runs and non-ascending neighbours; else, among the samples whose common sites come in another order than
    the shortest sample's (the lowest index among equals)"""
    for s, sites in enumerate(samples):
        seen = set()
        for i, k in enumerate(sites):
            if i == 0 or sites[i - 1][0] != k[0]:
                if k[0] in seen:
                    return ("refused", SPLIT, s, i)
                seen.add(k[0])
            elif not sites[i - 1][1:] < k[1:]:
                return ("refused", NOT_ASCENDING, s, i)
    common = set(samples[0])
    for sites in samples[1:]:
        common &= set(sites)
    probe = min(range(len(samples)), key=lambda s: (len(samples[s]), s))
    order = [k for k in samples[probe] if k in common]
    for s, sites in enumerate(samples):
        where = {k: i for i, k in enumerate(sites)}
        src = [where[k] for k in order]
        bad = [src[k] for k in range(1, len(src)) if src[k] <= src[k - 1]]
        if bad:
            return ("refused", NOT_COORDERED, s, min(bad))
    return ("ok", [np.array([k in common for k in sites], dtype=np.uint8) for sites in samples], len(common))


def ordered(keys, chrom_order):
    rank = {c: i for i, c in enumerate(chrom_order)}
    return sorted(keys, key=lambda k: (rank[k[0]], k[1], k[2], k[3]))


def make_case(rng, n_samples, n_common, n_extra, chrom_order=(1, 10, 2), lonely=None, drop_first=False, drop_last=False):
    """n_samples well ordered, co-ordered samples with exactly n_common common keys and n_extra keys that at least one sample
    has and at least one lacks (none with one sample); starts are drawn from a small range, so keys that differ only in end
    or only in strand are frequent.  lonely: a chromosome (behind the others) whose keys are all extra: present in some
    samples, common in none.  drop_first / drop_last: the lowest / highest key of all is an extra."""
    chroms = list(chrom_order)
    span = max(8, (n_common + n_extra) // (2 * len(chroms)))
    keys = set()
    while len(keys) < n_common + (n_extra if n_samples > 1 else 0):
        start = int(rng.integers(1, span + 1))
        keys.add((int(chroms[int(rng.integers(len(chroms)))]), start, start + int(rng.integers(0, 3)), int(rng.integers(0, 3))))
    keys = ordered(keys, chroms)
    extra = set()
    if n_samples > 1 and n_extra:
        pick = set(rng.choice(len(keys), size=n_extra, replace=False).tolist())
        forced = ([0] if drop_first else []) + ([len(keys) - 1] if drop_last else [])
        for f in forced:
            if f not in pick:
                pick.remove(next(i for i in sorted(pick) if i not in forced))
                pick.add(f)
        extra = {keys[i] for i in pick}
    samples = [[] for _ in range(n_samples)]
    for j, k in enumerate(keys):
        if k in extra:
            has = rng.random(n_samples) < 0.5
            if has.all() or not has.any():
                has[:] = True
                has[int(rng.integers(n_samples))] = False
            if (drop_first and j == 0) or (drop_last and j == len(keys) - 1):
                has[:] = True
                has[int(rng.integers(n_samples))] = False               # a first / last site of all but one sample
        else:
            has = np.ones(n_samples, dtype=bool)
        for s in np.flatnonzero(has):
            samples[s].append(k)
    if lonely is not None and n_samples > 1:
        absent = int(rng.integers(n_samples))
        for s in range(n_samples):
            if s != absent:
                samples[s] += [(lonely, 5 + 3 * i, 6 + 3 * i, i % 3) for i in range(1 + s)]
    return samples


def coverage(samples, keep):
    """(samples whose first site is dropped, whose last site is dropped, (sample, chromosome) runs dropped whole)"""
    first = sum(1 for s, k in zip(samples, keep) if len(s) and not k[0])
    last = sum(1 for s, k in zip(samples, keep) if len(s) and not k[-1])
    whole = 0
    for s, k in zip(samples, keep):
        for c in {key[0] for key in s}:
            whole += not any(k[i] for i, key in enumerate(s) if key[0] == c)
    return first, last, whole


def refusal_cases(rng):
    """[(name, samples, kind)]: each kind of refusal three times or more, the offending site first, last and in between"""
    cases = []
    for rep in range(3):
        base = make_case(rng, 3, 40 + rep, 12)
        chroms = [k[0] for k in base[1]]
        b = [list(s) for s in base]                                      # a run split by another chromosome's
        second = chroms.index(10)
        b[1] = b[1][:2] + b[1][second:second + 2] + b[1][2:second] + b[1][second + 2:]
        cases.append((f"split {rep}", b, SPLIT))
        b = [list(s) for s in base]                                      # the second run is the last site alone
        b[2] = b[2] + [(1, 4000, 4000, 0)]
        cases.append((f"split at the last site {rep}", b, SPLIT))
        b = [list(s) for s in base]                                      # a descending neighbour
        i = 5 + rep
        while b[0][i][0] != b[0][i + 1][0]:
            i += 1
        b[0][i], b[0][i + 1] = b[0][i + 1], b[0][i]
        cases.append((f"descending {rep}", b, NOT_ASCENDING))
        b = [list(s) for s in base]                                      # a duplicate key, at the last site
        b[2] = b[2] + [b[2][-1]]
        cases.append((f"duplicate last {rep}", b, NOT_ASCENDING))
        b = [list(s) for s in base]                                      # ... at site 1: the lowest index that can descend
        b[rep] = [b[rep][0]] + b[rep]
        cases.append((f"duplicate first {rep}", b, NOT_ASCENDING))
        b = [list(s) for s in base]                                      # the runs in another order in one sample
        longest = max(range(3), key=lambda s: len(b[s]))
        rest = [k for k in b[longest] if k[0] != 2]
        b[longest] = [k for k in b[longest] if k[0] == 2] + rest
        cases.append((f"run order {rep}", b, NOT_COORDERED))
    return cases
