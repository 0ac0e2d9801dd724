"""Genomic tiles (alphabeta_rs_amd/csrc/abn_tiles.hpp) as a plain numpy / Python model, and the inputs the tile tests
share.  A column has one key (chromosome, start); the columns of a chromosome form one run, ascending in start; a tile
(chromosome, start, end) is half-open on a site's start and becomes a column range by two searchsorted calls inside the
chromosome's run.  The folds are Python float loops (IEEE f64 adds in file order: the host's bits, src/pedigree.rs:159-172),
D comes from the code bytes (src/pedigree.rs:245-251), and fixed_intervals restates abn_tiles_set_fixed.  No product code."""
import struct

import numpy as np

import _parse_model as P

FILTER = 0.99
COUNTED = 0x40            # kCodeCounted
POS_END = 1 << 32         # the highest tile bound
CHROM = {"M": 256, "C": 257}
STRAND = {"+": 0, "-": 1}
LAST = 4294967295         # the highest start a site can have


def chromosome_key(name):
    return CHROM[name] if name in CHROM else int(name)


def chromosome_name(key):
    return {256: "M", 257: "C"}.get(int(key), str(int(key)))


# ---------------------------------------------------------------- the model
def runs_of(chromosome, start):
    """[(chromosome, first column, columns, start of the last column)] in run order"""
    chromosome = np.asarray(chromosome)
    runs, first = [], 0
    for k in range(1, len(chromosome) + 1):
        if k == len(chromosome) or chromosome[k] != chromosome[first]:
            runs.append((int(chromosome[first]), first, k - first, int(start[k - 1])))
            first = k
    return runs


def search(chromosome, start, tiles):
    """tiles = (chromosome, start, end) arrays -> (begin, end) int64: the columns with tile start <= start < tile end inside
    the chromosome's run; [0, 0) for a chromosome without a run; begin = end for end <= start"""
    start = np.asarray(start, dtype=np.int64)
    by_chrom = {c: (f, f + n) for c, f, n, _ in runs_of(chromosome, start)}
    begin, end = [], []
    for c, lo, hi in zip(*(np.asarray(a).tolist() for a in tiles)):
        if c not in by_chrom:
            begin.append(0), end.append(0)
            continue
        f, e = by_chrom[c]
        b = f + int(np.searchsorted(start[f:e], lo, side="left"))
        begin.append(b)
        end.append(b if hi <= lo else f + int(np.searchsorted(start[f:e], hi, side="left")))
    return np.array(begin, dtype=np.int64), np.array(end, dtype=np.int64)


def fixed_intervals(runs, size, step=0):
    """abn_tiles_set_fixed: for every run in run order the tiles k = 0 .. ceil((last_start + 1) / step) - 1,
    [k step, k step + size), the end capped at 2^32"""
    step = step or size
    chrom, lo, hi = [], [], []
    for c, _, _, last in runs:
        for k in range(-(-(last + 1) // step)):
            chrom.append(c), lo.append(k * step), hi.append(min(k * step + size, POS_END))
    return np.array(chrom, dtype=np.int32), np.array(lo, dtype=np.int64), np.array(hi, dtype=np.int64)


def fold(counted, level, b, e):
    """(sum as its 8 bytes, kept) of the columns [b, e): `if counted { sum += level; kept += 1 }` from 0.0"""
    s, k = 0.0, 0
    for c, x in zip(counted[b:e].tolist(), level[b:e].tolist()):
        if c:
            s += x
            k += 1
    return struct.pack("<d", s), k


def folds(columns, begin, end):
    """columns = aligned(...)'s samples -> (sum bytes [n][T], kept [n][T])"""
    sums = [[fold(s["counted"], s["level"], b, e) for b, e in zip(begin.tolist(), end.tolist())] for s in columns]
    return [[x[0] for x in row] for row in sums], np.array([[x[1] for x in row] for row in sums], dtype=np.int64).reshape(len(columns), len(begin))


def pairwise(columns, begin, end):
    """(diff, both uint64 [T x pairs], dvalue [T x pairs]) from the fields (status, 3 when filtered): a site is compared
    where neither sample's is filtered (src/pedigree.rs:245-251), D = diff / (2 both)"""
    n, T = len(columns), len(begin)
    pairs = [(i, j) for i in range(n) for j in range(i + 1, n)]
    diff, both = np.zeros((T, len(pairs)), dtype=np.uint64), np.zeros((T, len(pairs)), dtype=np.uint64)
    for t, (b, e) in enumerate(zip(begin.tolist(), end.tolist())):
        for p, (i, j) in enumerate(pairs):
            a, c = columns[i]["field"][b:e].astype(np.int64), columns[j]["field"][b:e].astype(np.int64)
            ok = (a < 3) & (c < 3)
            both[t, p] = int(ok.sum())
            diff[t, p] = int(np.abs(a - c)[ok].sum())
    with np.errstate(all="ignore"):
        dvalue = diff.astype(np.float64) / (2.0 * both.astype(np.float64))
    return diff, both, dvalue


# ---------------------------------------------------------------- inputs
def master_sites():
    """The sites of the test methylomes, ~1500: three chromosome runs in the order 2, 1, C (run order is not the order of
    the chromosome keys 2, 1, 257); positions 10 apart with a gap of millions inside chromosome 1; both strands at one start
    in a few places; the last site of the last run at start 4294967295.  -> [(chromosome name, start, strand)]"""
    rows = []
    for k in range(520):                                   # run "2": columns 0 .. 529
        rows.append(("2", 10 * (k + 1), "+-"[k % 2]))
        if k in (300, 301, 400, 519):                      # both strands at one start; 519: the run's last start
            rows[-1] = ("2", 10 * (k + 1), "+")
            rows.append(("2", 10 * (k + 1), "-"))
    for k in range(480):                                   # run "1": a gap of 3 000 000 behind its 100th site
        pos = 7 * (k + 1) + (3000000 if k >= 100 else 0)
        rows.append(("1", pos, "+"))
        if k in (99, 100, 250):
            rows.append(("1", pos, "-"))
    for k in range(490):                                   # run "C"
        rows.append(("C", 1000 + 3 * k, "-+"[k % 2]))
    rows.append(("C", LAST, "+"))
    return rows


def sample_values(rows, seed, nan_at=None):
    """per site of one sample: the text tokens (posterior, status, level) -> dict of lists.  Posteriors on both sides of the
    filter and at it, levels of -0.0 among the others; nan_at: that site's posterior is `nan` (the host decides the line:
    not filtered, and not counted)"""
    rng = np.random.default_rng(seed)
    pm = [("0.9999", "0.99", f"{rng.random():.4f}", "0.5", "0.9999")[int(rng.integers(5))] for _ in rows]
    st = ["UIM"[int(rng.integers(3))] for _ in rows]
    ml = ["-0.0" if rng.integers(6) == 0 else f"{rng.random():.4f}" for _ in rows]
    if nan_at is not None:
        pm[nan_at] = "nan"
    return {"pm": pm, "st": st, "ml": ml}


def methylome_text(rows, values, keep=None):
    """the methylome text of the sites `keep` (indices into rows; None: all), rows of other contexts (no site) in between"""
    out = [P.HEADER]
    for i in (range(len(rows)) if keep is None else keep):
        c, pos, strand = rows[i]
        if i % 5 == 0:
            out.append(P.cg_line(chrom=c, pos=str(pos), ctx="CHH", tri="CCT") + "\n")
        out.append(P.cg_line(chrom=c, pos=str(pos), strand=strand, pm=values["pm"][i], st=values["st"][i], ml=values["ml"][i],
                             tri="CGA") + "\n")
    return "".join(out).encode()


def aligned(rows, values_per_sample, keep_per_sample, align):
    """The columns after the alignment.  keep_per_sample[s]: the sorted site indices sample s holds.  align "none": every
    sample holds the same sites; "position": the sites all hold; "union": the sites any holds, a filtered, uncounted
    placeholder where a sample lacks one.  -> (chromosome int32, start int64, strand uint8, [per sample {field, counted, level, code}])"""
    held = [set(k) for k in keep_per_sample]
    if align == "none":
        assert all(h == held[0] for h in held)
        cols = sorted(held[0])
    elif align == "position":
        cols = sorted(set.intersection(*held))
    else:
        cols = sorted(set.union(*held))
    chrom = np.array([chromosome_key(rows[i][0]) for i in cols], dtype=np.int32)
    start = np.array([rows[i][1] for i in cols], dtype=np.int64)
    strand = np.array([STRAND[rows[i][2]] for i in cols], dtype=np.uint8)
    samples = []
    for v, h in zip(values_per_sample, held):
        pm = np.array([float(v["pm"][i]) if i in h else 0.0 for i in cols])
        present = np.array([i in h for i in cols], dtype=bool)
        status = np.array(["UIM".index(v["st"][i]) for i in cols], dtype=np.uint8)
        with np.errstate(invalid="ignore"):
            filtered = ~present | (pm < FILTER)
            counted = present & (pm >= FILTER)
        level = np.array([float(v["ml"][i]) if i in h else 0.0 for i in cols])
        field = np.where(filtered, 3, status).astype(np.uint8)
        code = (np.where(present, status, 0) | np.where(filtered, 0x80, 0) | np.where(counted, COUNTED, 0)).astype(np.uint8)
        samples.append({"field": field, "counted": counted, "level": level, "code": code})
    return chrom, start, strand, samples


def tile_list(rows):
    """The explicit tiles of the tests, over the sites of master_sites() -> (chromosome int32, start int64, end int64) and
    the names of the cases, tile by tile"""
    s2 = [r[1] for r in rows if r[0] == "2"]               # starts of run "2", columns 0 ..
    s1 = [r[1] for r in rows if r[0] == "1"]
    tiles = [
        ("first column on", "2", 0, s2[63]),                        # begins at column 0: 63 columns
        ("64 columns", "2", s2[7], s2[7 + 64]),                     # begin 7: no multiple of 16
        ("65 columns", "2", s2[70] - 3, s2[70 + 65] - 3),
        ("200 columns", "2", s2[33], s2[33 + 200]),
        ("one column", "2", s2[5], s2[5] + 1),
        ("no column", "2", s2[5] + 1, s2[6]),                       # between two sites
        ("end <= start", "2", 500, 500),
        ("end < start", "2", 900, 100),
        ("both strands", "2", s2[300], s2[300] + 1),                # the two sites at one start
        ("run's last column", "2", s2[-1] - 95, s2[-1] + 1),
        ("behind the run", "2", s2[-1] + 1, s2[-1] + 5000),
        ("over the gap", "1", s1[90], s1[110]),
        ("whole run 1", "1", 0, POS_END),
        ("no such chromosome", "7", 0, POS_END),
        ("mitochondrial, absent", "M", 5, 50000),
        ("up to 2^32", "C", LAST - 10, POS_END),                    # holds the site at 4294967295
        ("at 2^32", "C", POS_END, POS_END),
        ("C from 0", "C", 0, 1000 + 3 * 129 + 1),                   # begin: the first column of the last run
        ("overlaps the 200", "2", s2[100], s2[260]),
    ]
    names = [t[0] for t in tiles]
    return (np.array([chromosome_key(t[1]) for t in tiles], dtype=np.int32), np.array([t[2] for t in tiles], dtype=np.int64),
            np.array([t[3] for t in tiles], dtype=np.int64)), names
