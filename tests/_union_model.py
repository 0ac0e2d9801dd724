"""What the tests of the union step share (tests/test_sites_union_cpu.py, tests/test_sites_union_gpu.py): the definition of
include/abneutral.h ("methylomes aligned on the union of their sites") spelled out in Python with sets, dictionaries and a
sort of key tuples — no search, no table of runs, no owners — on the samples of _common_model.make_case."""
import numpy as np

import _common_model as X

SPLIT, NOT_ASCENDING, BAD_KEY, RUN_ORDER = 1, 2, 3, 5               # CommonRefusal.kind; 5: csrc/abn_sites_union.hpp
WORDS = {SPLIT: "split run", NOT_ASCENDING: "not ascending", RUN_ORDER: "run order"}
PLACEHOLDER_CODE = 0x80


def runs_of(sites):
    """the chromosomes of a well ordered sample in run order"""
    out = []
    for k in sites:
        if not out or out[-1] != k[0]:
            out.append(k[0])
    return out


def chromosome_order(samples):
    """the reference sample's run order (most runs, the lowest index among equals), then what it lacks as first met"""
    runs = [runs_of(s) for s in samples]
    ref = max(range(len(samples)), key=lambda s: (len(runs[s]), -s))
    order = list(runs[ref])
    for r in runs:
        order += [c for c in r if c not in order]
    return order, runs


def model(samples):
    """-> ("ok", dest per sample (uint32), n_union, union keys in order) or ("refused", kind, sample, site): the lowest
    offending site of the whole input among split runs and non-ascending neighbours; else the first site of the first run,
    in the lowest sample that has one, whose chromosome stands in the union order before the one of the run in front"""
    well = X.model(samples)
    if well[0] == "refused" and well[1] in (SPLIT, NOT_ASCENDING):
        return well
    order, runs = chromosome_order(samples)
    pos = {c: i for i, c in enumerate(order)}
    for s, r in enumerate(runs):
        for k in range(1, len(r)):
            if pos[r[k]] < pos[r[k - 1]]:
                return ("refused", RUN_ORDER, s, next(i for i, key in enumerate(samples[s]) if key[0] == r[k]))
    union = sorted(set().union(*map(set, samples)), key=lambda k: (pos[k[0]], k[1], k[2], k[3]))
    rank = {k: u for u, k in enumerate(union)}
    return ("ok", [np.array([rank[k] for k in s], dtype=np.uint32) for s in samples], len(union), union)


def padded(samples, union, payload=None):
    """every sample's row over the union: [(key, payload or None)] — None where the sample lacks the key.  payload:
    per sample, a list parallel to its sites"""
    rows = []
    for s, sites in enumerate(samples):
        mine = {k: (payload[s][i] if payload is not None else i) for i, k in enumerate(sites)}
        rows.append([(k, mine.get(k)) for k in union])
    return rows


def coverage(samples, union):
    """what a batch of cases must exercise: (keys only the last sample holds, keys whose owner — the lowest sample that
    holds it — is sample 4 or above while a later sample holds it too, (sample, chromosome) pairs without a site, samples
    whose first union site is a placeholder, samples whose last one is)"""
    sets = [set(s) for s in samples]
    n = len(samples)
    holders = {k: [s for s in range(n) if k in sets[s]] for k in union}
    last_only = sum(1 for h in holders.values() if n > 1 and h == [n - 1])
    second_group = sum(1 for h in holders.values() if h[0] >= 4 and len(h) > 1)
    chroms = {k[0] for k in union}
    no_site = sum(1 for s in sets for c in chroms if not any(k[0] == c for k in s))
    first = sum(1 for s in sets if union and union[0] not in s)
    last = sum(1 for s in sets if union and union[-1] not in s)
    return last_only, second_group, no_site, first, last


def run_order_cases():
    """[(name, samples, sample, site)]: the run-order refusal where the run reported is the sample's second (its first run
    is the one displaced), a middle and the last run; a chromosome the reference lacks; two offenders, the lowest wins"""
    key = lambda c, i: (c, 10 + i, 11 + i, i % 3)
    run = lambda c, n, at=0: [key(c, at + i) for i in range(n)]
    ref = run(1, 5) + run(10, 4) + run(2, 6) + run(7, 3)
    return [
        ("the first run displaced", [ref, run(2, 3) + run(1, 4) + run(10, 2)], 1, 3),
        ("a middle run", [ref, run(1, 2) + run(2, 3) + run(10, 4) + run(7, 1)], 1, 5),
        ("the last run", [run(1, 3) + run(2, 2) + run(10, 1), ref], 0, 5),
        ("the reference is the lowest of the longest", [run(2, 2) + run(1, 2), run(1, 2) + run(2, 2)], 1, 2),
        ("a chromosome the reference lacks", [run(5, 2) + run(1, 3), ref, run(1, 2) + run(5, 1)], 0, 2),
        ("two offenders", [ref, run(1, 3), run(10, 2) + run(1, 2), run(7, 1) + run(2, 4)], 2, 2),
    ]


UNION_COUNTS = (0, 1, 63, 64, 65, 255, 256, 257, 1025)
SAMPLE_COUNTS = (1, 2, 3, 5, 6, 9)              # six and nine: a key's owner in the second and third search group


def generated_cases():
    """108 of them: (name, samples, n_common + n_extra).  Without the lonely chromosome that sum is n_union (with one
    sample, which has no extras, n_common is)."""
    rng = np.random.default_rng(20261020)
    for total in UNION_COUNTS:
        for n_samples in SAMPLE_COUNTS:
            for lonely in (None, 30):
                extra = 0 if n_samples == 1 else min(total, (0, 7, 40)[(total + n_samples) % 3])
                samples = X.make_case(rng, n_samples, total - extra, extra,
                                      chrom_order=((1, 10, 2), (2, 1, 257, 256))[(n_samples + (lonely is None)) % 2],
                                      lonely=lonely, drop_first=total % 3 == 0, drop_last=total % 3 == 1)
                yield (total, n_samples, lonely), samples, total
