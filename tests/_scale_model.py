"""What the scale tier shares (tests/test_scale_cpu.py, tests/test_scale_gpu.py): inputs past one scan workgroup's first
trip that carry their own truth.  The reference is the arrays a text was written from — never one of the project's
parsers — and floats are float(token), correctly rounded like strtod.  The sizes are derived from the kernels' constants,
kept here beside their C++ names; tests/test_scale_cpu.py reads them out of the headers again."""
from functools import lru_cache

import numpy as np

import _parse_model as P

# name here -> (header under alphabeta_rs_amd/csrc, C++ name)
CONSTANTS = {
    "PARSE_THREADS": ("abn_parse_kernels.hpp", "kParseThreads"),
    "PARSE_PIECE_BYTES": ("abn_parse_kernels.hpp", "kParsePieceBytes"),
    "PARSE_SCAN_THREADS": ("abn_parse_kernels.hpp", "kParseScanThreads"),
    "PARSE_RUN": ("abn_parse_kernels.hpp", "kParseRun"),
    "SPLIT_THREADS": ("abn_sites_split.hpp", "kSplitThreads"),
    "MERGE_THREADS": ("abn_sites_merge.hpp", "kMergeThreads"),
    "MERGE_FLAG_BLOCKS": ("abn_sites_merge.hpp", "kMergeFlagBlocks"),
    "COMMON_THREADS": ("abn_sites_common.hpp", "kCommonThreads"),
}
PARSE_THREADS = 256          # kParseThreads: lanes of K1 / K2, a 16-byte piece each
PARSE_PIECE_BYTES = 16       # kParsePieceBytes
PARSE_SCAN_THREADS = 1024    # kParseScanThreads: lanes of abn_parse_scan_kernel
PARSE_RUN = 256              # kParseRun: lines per workgroup of K3
SPLIT_THREADS = 256          # kSplitThreads: records per workgroup of the split
MERGE_THREADS = 256          # kMergeThreads
MERGE_FLAG_BLOCKS = 256      # kMergeFlagBlocks: workgroups of abn_sites_flagged_kernel at most
COMMON_THREADS = 256         # kCommonThreads: lanes of abn_common_scan_kernel, and sites per block of its callers

PARSE_BLOCK_BYTES = PARSE_THREADS * PARSE_PIECE_BYTES             # text per workgroup of K1
SCAN_RUNS = PARSE_SCAN_THREADS * PARSE_RUN                        # 262 144 lines: the runs one scan lane each
FLAG_TRIP = MERGE_FLAG_BLOCKS * MERGE_THREADS                     # 65 536 records: the flag kernel's first trip
COMMON_TRIP = COMMON_THREADS * COMMON_THREADS                     # 65 536 sites: one block per lane of the common scan
SCALE_LINES = SCAN_RUNS + PARSE_RUN + 1                           # 262 401: 1026 runs, per = 2
SLAB_BYTES = 5 << 20                                              # test 2's slabs: more than 1024 K1 blocks each

CONTEXTS = ("CG", "CHG", "CHH")
CHROMOSOMES = (("1", 1), ("10", 10), ("2", 2), ("M", 256), ("C", 257))     # file order: not the order of the keys
LONG = "0.999900000000000000000"       # 21 digits: the device defers the line, the host reads 0.9999
DEFERRED_TOKENS = (LONG, "1e23")
BOUNDARY_TOKENS = ("9007199254740992", "9007199254740992e22", "1e22", "1e-22", "0.0000000000000000000001", "-0.0", "007.2500",
                   ".5", "5.")
POOL_CLASSES = ("four decimals", "1 to 15 digits", "16 digits", "exponent")     # (a) to (d); 4: the boundary tokens
SITE_KEYS = ("line", "chromosome", "start", "end", "strand", "posteriormax", "status", "meth_lvl", "status_flag", "context")


def ceil_div(a, b):
    return -(-a // b)


def scan_per(n, threads):
    """the serial slice of a lane of the two-level scans: `per` of abn_parse_scan_kernel / abn_common_scan_kernel"""
    return ceil_div(n, threads)


# ---------------------------------------------------------------- the float tokens
@lru_cache(maxsize=None)
def token_pool(per_class=1000):
    """-> (tokens, float(token) per token, class per token): per_class tokens of each of POOL_CLASSES, every one a token
    abn_parse_f64 must decide (at most 2^53 as an integer, the decimal exponent within +-22), and BOUNDARY_TOKENS"""
    rng = np.random.default_rng(20261101)
    digits = lambda n: "".join(map(str, rng.integers(0, 10, size=n).tolist()))
    tokens, cls = [], []
    for v in rng.random(per_class).tolist():                                   # (a)
        tokens.append(f"{v:.4f}")
    for _ in range(per_class):                                                 # (b)
        n = int(rng.integers(1, 16))
        zeros = int(rng.integers(0, min(3, 16 - n)))                           # trailing zeros count as digits written
        d = digits(n)
        at = int(rng.integers(0, n + 1))
        tok = d[:at] + "." + d[at:] + "0" * zeros
        if at == n and zeros == 0 and n > 0 and rng.integers(2):
            tok = d                                                            # no point at all
        if rng.integers(4) == 0:
            tok = "0" * int(rng.integers(1, 3)) + tok
        if rng.integers(4) == 0:
            tok = "-" + tok
        tokens.append(tok)
    for _ in range(per_class):                                                 # (c)
        d = str(int(rng.integers(10 ** 15, (1 << 53) + 1)))
        at = int(rng.integers(0, 17))
        tokens.append("0." + d if at == 0 else (d if at == 16 else d[:at] + "." + d[at:]))
    for _ in range(per_class):                                                 # (d)
        w = int(rng.integers(0, min(10 ** int(rng.integers(1, 17)), (1 << 53) + 1)))
        x = int(rng.integers(-22, 23))
        tokens.append(f"{w}{'eE'[int(rng.integers(2))]}{('', '+')[int(rng.integers(2))] if x >= 0 else ''}{x}")
    cls = np.repeat(np.arange(4, dtype=np.uint8), per_class)
    tokens += list(BOUNDARY_TOKENS)
    cls = np.concatenate([cls, np.full(len(BOUNDARY_TOKENS), 4, dtype=np.uint8)])
    return tuple(tokens), np.array([float(t) for t in tokens]), cls


# ---------------------------------------------------------------- one text past every parse threshold
def _write(chrom_name, start, strand, ctx_name, pm_tok, status_chr, ml_tok, ten):
    """the lines of a methylome (first and second format: nine fields, or ten with the trinucleotide), tokens pre-made"""
    return [f"{c}\t{s}\t{sd}\t{cx}\t3\t8\t{pm}\t{st}\t{ml}\tCGA" if t else f"{c}\t{s}\t{sd}\t{cx}\t3\t8\t{pm}\t{st}\t{ml}"
            for c, s, sd, cx, pm, st, ml, t in zip(chrom_name, start, strand, ctx_name, pm_tok, status_chr, ml_tok, ten)]


def _runs(n, rng, shares):
    """the run of every one of n lines: len(shares) chromosome runs in file order, no run boundary on a multiple of 256"""
    cuts = np.floor(np.cumsum(shares)[:-1] / np.sum(shares) * n).astype(np.int64)
    cuts += (cuts % PARSE_RUN == 0) * 7 + rng.integers(1, 5, size=len(cuts))
    return np.searchsorted(cuts, np.arange(n), side="right")


def _ascending_starts(run, rng, top=40):
    """starts ascending inside every run, from a small number again at every run's first line"""
    step = rng.integers(1, top, size=len(run)).astype(np.int64)
    total = np.cumsum(step)
    first = np.flatnonzero(np.diff(run, prepend=-1))
    return total - np.repeat(total[first] - step[first], np.diff(np.append(first, len(run))))


@lru_cache(maxsize=2)
def scale_text(n_lines=SCALE_LINES, seed=3):
    """-> (text, truth, planted).  truth: the arrays of every site of the text under all three contexts (SITE_KEYS; `decided`:
    the device decides the line; `pm_class`, `ml_class`: the pool class of its float tokens), file order.  planted: the file
    lines of the `deferred` lines (with `deferred_offset`, `deferred_length`, `deferred_context`), the `rejected` lines (no
    site for any parser: start is `1x`) and the `flagged` ones (status byte X, all CG).  Data line d is file line d + 1 and
    lane d % 256 of K3's run d // 256.  The default seed gives 3090 K1 blocks: no multiple of the scan's per = 4, so the
    last slice is ragged (the tests assert it)."""
    rng = np.random.default_rng(seed)
    tokens, values, classes = token_pool()
    n = n_lines
    assert n > SCAN_RUNS + PARSE_RUN
    d_all = np.arange(n)
    run = _runs(n, rng, (30, 25, 20, 15, 10))
    start = _ascending_starts(run, rng)
    strand = rng.integers(0, 2, size=n)
    ctx = rng.integers(0, 3, size=n)
    status = rng.integers(0, 3, size=n)
    ten = d_all % 3 != 0
    pm_i, ml_i = rng.integers(0, len(tokens), size=(2, n))
    # the lines that must be deferred whatever the mask: CG by force
    last_run = (n - 1) // PARSE_RUN - 1                                        # run 1024 of 1026: the last full one
    edges = sorted({0, n - 1} | {r * PARSE_RUN + j for r in (0, last_run) for j in (255, 256, 257) if r * PARSE_RUN + j < n})
    # rejected lines around the run boundaries next to those (a line cannot be both): runs 1 | 2 and 1023 | 1024
    around = sorted({b + j for b in (2 * PARSE_RUN, last_run * PARSE_RUN) for j in (-1, 0, 1)})
    ctx[edges + around] = 0
    rejected = np.zeros(n, dtype=bool)
    rejected[around] = True
    free = np.setdiff1d(d_all, edges + around)
    rejected[rng.choice(free, size=30, replace=False)] = True
    deferred = np.zeros(n, dtype=bool)
    deferred[edges] = True
    # about 0.1 % more at random, but no more than leave the all-context parse over 1024 x 256 records on the device: the
    # split's threshold, which the lines that are no record count against (180 of the 262 401 lines, 0.07 %)
    spare = n - (PARSE_SCAN_THREADS * SPLIT_THREADS + 32) - len(edges) - 3 - int(rejected.sum())
    assert spare >= n // 2000
    free = free[~rejected[free]]
    deferred[rng.choice(free, size=min(n // 1000, spare), replace=False)] = True
    cg_sites = np.flatnonzero((ctx == 0) & ~rejected)
    assert len(cg_sites) > FLAG_TRIP + 2 * len(edges) + n // 1000
    deferred[cg_sites[FLAG_TRIP - 1:FLAG_TRIP + 2]] = True                    # CG sites 65 535, 65 536, 65 537
    cg_records = np.flatnonzero((ctx == 0) & ~rejected & ~deferred)            # what the CG-only parse leaves on the device
    assert len(cg_records) > FLAG_TRIP + 1
    flagged = np.zeros(n, dtype=bool)
    flagged[cg_records[[0, FLAG_TRIP - 1, FLAG_TRIP, -1]]] = True
    flagged[rng.choice(cg_records, size=50, replace=False)] = True
    status[flagged] = 0                                                        # a status byte that is none of M, I, U reads as U
    # the text
    pm_tok = [tokens[i] for i in pm_i.tolist()]
    ml_tok = [tokens[i] for i in ml_i.tolist()]
    pm, ml = values[pm_i], values[ml_i]
    for k, d in enumerate(np.flatnonzero(deferred).tolist()):
        tok = DEFERRED_TOKENS[k % 2]
        if (k // 2) % 2:
            ml_tok[d], ml[d] = tok, float(tok)
        else:
            pm_tok[d], pm[d] = tok, float(tok)
    start_tok = list(map(str, start.tolist()))
    for d in np.flatnonzero(rejected).tolist():
        start_tok[d] = "1x"
    status_chr = np.where(flagged, "X", np.array(list("UIM"))[status]).tolist()
    lines = _write(np.array([c for c, _ in CHROMOSOMES])[run].tolist(), start_tok, np.array(["+", "-"])[strand].tolist(),
                   np.array(CONTEXTS)[ctx].tolist(), pm_tok, status_chr, ml_tok, ten.tolist())
    text = (P.HEADER + "\n".join(lines) + "\n").encode()
    length = np.fromiter(map(len, lines), dtype=np.int64, count=n)
    offset = len(P.HEADER) + np.cumsum(length + 1) - (length + 1)
    site = ~rejected
    truth = {"line": (d_all + 1)[site].astype(np.int64),
             "chromosome": np.array([k for _, k in CHROMOSOMES], dtype=np.int32)[run][site],
             "start": start[site].astype(np.uint32), "end": (start[site] + 1).astype(np.uint32),
             "strand": strand[site].astype(np.uint8), "posteriormax": pm[site], "status": status[site].astype(np.uint8),
             "meth_lvl": ml[site], "status_flag": flagged[site].astype(np.uint8), "context": ctx[site].astype(np.uint8),
             "decided": ~deferred[site], "pm_class": classes[pm_i][site], "ml_class": classes[ml_i][site]}
    dl = np.flatnonzero(deferred)
    planted = {"deferred": (dl + 1).astype(np.int64), "deferred_offset": offset[dl], "deferred_length": length[dl],
               "deferred_context": ctx[dl].astype(np.uint8), "rejected": (np.flatnonzero(rejected) + 1).astype(np.int64),
               "flagged": (np.flatnonzero(flagged) + 1).astype(np.int64), "n_lines": n + 1}
    for a in list(truth.values()) + [v for v in planted.values() if isinstance(v, np.ndarray)]:
        a.setflags(write=False)
    return text, truth, planted


def in_mask(context, mask):
    return ((mask >> np.asarray(context, dtype=np.int64)) & 1).astype(bool)


def truth_under(truth, mask, decided_only=False):
    """the sites of the contexts of `mask`, in file order; decided_only: those the device decides"""
    pick = in_mask(truth["context"], mask)
    if decided_only:
        pick &= truth["decided"]
    return {k: v[pick] for k, v in truth.items()}


def deferred_under(planted, mask):
    """{line, offset, length} of the planted lines a parse under `mask` defers: a line of another context is no site before
    any float field is read"""
    pick = in_mask(planted["deferred_context"], mask)
    return {"line": planted["deferred"][pick], "offset": planted["deferred_offset"][pick], "length": planted["deferred_length"][pick]}


def slabs(text, slab_bytes):
    """[(begin, end)] of the slabs abn_sites_parse cuts: behind the last line end of every slab_bytes bytes"""
    out, at = [], 0
    while at < len(text):
        end = len(text) if not slab_bytes or len(text) - at <= slab_bytes else text.rfind(b"\n", at, at + slab_bytes) + 1
        assert end > at
        out.append((at, end))
        at = end
    return out


def k1_blocks(n_bytes):
    return ceil_div(ceil_div(n_bytes, PARSE_PIECE_BYTES), PARSE_THREADS)


# ---------------------------------------------------------------- site keys of several samples
def composite(rank, start, end, strand):
    """one uint64 per key, ordered as (run rank, start, end, strand): end as its distance from start (below 2^18)"""
    start, end = np.asarray(start, dtype=np.int64), np.asarray(end, dtype=np.int64)
    span = end - start
    assert np.all((span >= 0) & (span < 1 << 18)) and np.all(np.asarray(rank) < 1 << 10) and np.all(np.asarray(strand) < 4)
    return (np.asarray(rank, dtype=np.uint64) << np.uint64(52) | start.astype(np.uint64) << np.uint64(20) |
            span.astype(np.uint64) << np.uint64(2) | np.asarray(strand, dtype=np.uint64))


def run_ranks(site_offset, chromosome):
    """chromosome key -> rank in the union's run order (include/abneutral.h): the run order of the sample with the most
    runs (the lowest among equals), then what it lacks as first met.  A loop over runs, not over sites."""
    runs = []
    for s in range(len(site_offset) - 1):
        c = np.asarray(chromosome[site_offset[s]:site_offset[s + 1]])
        runs.append(c[np.flatnonzero(np.r_[True, c[1:] != c[:-1]])].tolist() if len(c) else [])
    order = list(runs[max(range(len(runs)), key=lambda s: (len(runs[s]), -s))]) if runs else []
    for r in runs:
        order += [c for c in r if c not in order]
    rank = np.zeros(258, dtype=np.int64)
    rank[order] = np.arange(len(order))
    return rank


def expected_alignment(site_offset, chromosome, start, end, strand):
    """numpy set operations on the composite key -> (keep uint8 (S,), n_common, dest uint32 (S,), n_union) for well ordered,
    co-ordered samples: what Context.common_sites and Context.union_sites return"""
    off = np.asarray(site_offset, dtype=np.int64)
    key = composite(run_ranks(off, chromosome)[np.asarray(chromosome, dtype=np.int64)], start, end, strand)
    per_sample = [key[off[s]:off[s + 1]] for s in range(len(off) - 1)]
    common = per_sample[0]
    for k in per_sample[1:]:
        common = np.intersect1d(common, k, assume_unique=True)
    union = np.unique(key)
    keep = np.isin(key, common).astype(np.uint8)
    dest = np.searchsorted(union, key).astype(np.uint32)
    return keep, len(common), dest, len(union)


@lru_cache(maxsize=None)
def scale_keys(seed, universe, kept, disjoint_last_run=False):
    """len(kept) samples over one universe of `universe` keys in the chromosome run order of CHROMOSOMES, sample s keeping
    kept[s] of them: each drops its own random subset.  Keys as a methylome line spells them (end = start + 1, strand + or
    -), both strands at one start in places.  disjoint_last_run: every key of the last run is dropped by one sample at
    least.  -> (site_offset, chromosome, start, end, strand, universe index of every site, expected) with expected =
    {keep, n_common, dest, n_union}"""
    rng = np.random.default_rng(seed)
    run = _runs(universe, rng, (30, 25, 25, 19, 1))
    start = _ascending_starts(run, rng, top=30)
    strand = rng.integers(0, 2, size=universe)
    twice = np.flatnonzero((np.arange(universe - 1) % 20 == 3) & (run[:-1] == run[1:]))      # both strands at one start
    start[twice + 1], strand[twice], strand[twice + 1] = start[twice], 0, 1
    chrom = np.array([k for _, k in CHROMOSOMES], dtype=np.int32)[run]
    last = np.flatnonzero(run == run[-1])
    must_drop = rng.integers(0, len(kept), size=len(last))
    held = []
    for s, k in enumerate(kept):
        forced = last[must_drop == s] if disjoint_last_run else np.zeros(0, dtype=np.int64)
        assert len(forced) <= universe - k <= universe
        rest = np.setdiff1d(np.arange(universe), forced)
        drop = np.concatenate([forced, rng.choice(rest, size=universe - k - len(forced), replace=False)])
        held.append(np.setdiff1d(np.arange(universe), drop))
    index = np.concatenate(held)
    off = np.zeros(len(kept) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(h) for h in held])
    arrays = (off, chrom[index], start[index].astype(np.uint32), (start[index] + 1).astype(np.uint32), strand[index].astype(np.uint8))
    keep, n_common, dest, n_union = expected_alignment(*arrays)
    for a in arrays + (index, keep, dest):
        a.setflags(write=False)
    return (*arrays, index, {"keep": keep, "n_common": n_common, "dest": dest, "n_union": n_union})


def alignment_cases():
    """[(name, scale_keys arguments, `per` of abn_common_scan_kernel under position, under union)]: three samples past both
    thresholds, the boundary pairs either side of them (per = 1: the control), a sample other than sample 0 the shortest,
    and samples that share no site of the last chromosome run"""
    trip = COMMON_TRIP
    return [("three samples", dict(seed=41, universe=70000, kept=(68500, 68500, 68500)), 2, 4),
            ("no common site in the last run", dict(seed=42, universe=70000, kept=(68500, 68400, 68600), disjoint_last_run=True), 2, 4),
            ("probe of 65536, sample 1", dict(seed=43, universe=trip + 900, kept=(trip + 300, trip, trip + 500)), 1, 4),
            ("probe of 65537, sample 2", dict(seed=44, universe=trip + 900, kept=(trip + 300, trip + 2, trip + 1)), 2, 4),
            ("union of 32768 + 32768", dict(seed=45, universe=trip // 2 + 700, kept=(trip // 2, trip // 2)), 1, 1),
            ("union of 32769 + 32769", dict(seed=46, universe=trip // 2 + 700, kept=(trip // 2 + 1, trip // 2 + 1)), 1, 2)]


def alignment_pers(site_offset):
    """(`per` of the common scan under position: over the blocks of the shortest sample; under union: of all sites)"""
    n = np.diff(site_offset)
    return (scan_per(ceil_div(int(n.min()), COMMON_THREADS), COMMON_THREADS),
            scan_per(ceil_div(int(n.sum()), COMMON_THREADS), COMMON_THREADS))


def runs_of(chromosome, start):
    """[(chromosome, first column, columns, start of the last column)] in run order: _tiles_model.runs_of without the loop"""
    chromosome, start = np.asarray(chromosome), np.asarray(start)
    if len(chromosome) == 0:
        return []
    first = np.flatnonzero(np.r_[True, chromosome[1:] != chromosome[:-1]])
    end = np.append(first[1:], len(chromosome))
    return [(int(chromosome[f]), int(f), int(e - f), int(start[e - 1])) for f, e in zip(first, end)]


def keys_text(chromosome, start, strand, seed):
    """an all-CG methylome text of one sample's keys, posteriors and levels drawn from the four-decimal and 1-to-15-digit
    pool classes, a few deferred lines among them -> (text, {posteriormax, status, meth_lvl} per site)"""
    rng = np.random.default_rng(seed)
    tokens, values, classes = token_pool()
    plain, four = np.flatnonzero(classes <= 1), np.flatnonzero(classes == 0)
    n = len(start)
    pm_i, ml_i = plain[rng.integers(0, len(plain), size=n)], four[rng.integers(0, len(four), size=n)]
    pm_i[rng.random(n) < 0.5] = tokens.index("1e22")                           # half the sites pass the filter for sure
    ml_i[rng.random(n) < 0.1] = tokens.index("-0.0")                           # levels of one magnitude: every one shows in a sum
    status = rng.integers(0, 3, size=n)
    pm_tok, ml_tok = [tokens[i] for i in pm_i.tolist()], [tokens[i] for i in ml_i.tolist()]
    pm, ml = values[pm_i], values[ml_i]
    for d in sorted({d for d in (0, n - 1, FLAG_TRIP - 1, FLAG_TRIP) if 0 <= d < n} | set(rng.integers(0, n, size=40).tolist())):
        pm_tok[d], pm[d] = LONG, float(LONG)
    name = {k: c for c, k in CHROMOSOMES}
    lines = _write([name[c] for c in np.asarray(chromosome).tolist()], np.asarray(start).tolist(),
                   np.array(["+", "-"])[np.asarray(strand)].tolist(), ["CG"] * n, pm_tok, np.array(list("UIM"))[status].tolist(),
                   ml_tok, (np.arange(n) % 2 == 0).tolist())
    return (P.HEADER + "\n".join(lines) + "\n").encode(), {"posteriormax": pm, "status": status.astype(np.uint8), "meth_lvl": ml}


# ---------------------------------------------------------------- folds and codes, vectorised
def fold(counted, level):
    """(sum, kept) of `if counted { sum += level; kept += 1 }` from +0.0 in file order: np.cumsum adds in sequence, so the
    bits are the loop's (tests/test_scale_cpu.py pins it to _codes_model.fold and _tiles_model.fold)"""
    counted = np.asarray(counted, dtype=bool)
    x = np.asarray(level, dtype=np.float64)[counted]
    return (float(np.cumsum(np.concatenate([[0.0], x]))[-1]), int(counted.sum()))


def tile_search(chromosome, start, tiles):
    """two np.searchsorted per tile inside the chromosome's run -> (begin, end) int64; [0, 0) for a chromosome without one"""
    chromosome, start = np.asarray(chromosome), np.asarray(start, dtype=np.int64)
    first = np.flatnonzero(np.diff(chromosome, prepend=-1))
    by_chrom = {int(chromosome[f]): (int(f), int(e)) for f, e in zip(first, np.append(first[1:], len(chromosome)))}
    begin, end = [], []
    for c, lo, hi in zip(*(np.asarray(a).tolist() for a in tiles)):
        f, e = by_chrom.get(c, (0, 0))
        b = f + int(np.searchsorted(start[f:e], lo, side="left"))
        begin.append(b)
        end.append(b if hi <= lo else f + int(np.searchsorted(start[f:e], hi, side="left")))
    return np.array(begin, dtype=np.int64), np.array(end, dtype=np.int64)
