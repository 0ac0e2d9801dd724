"""A line-by-line Python restatement of the reference's `extract` stage, the model the window-extraction tests compare
the host parsers (alphabeta_rs_amd/host/windows_extract.hpp) and the device placement (abn_windows_*) against:
Gene::from_annotation_file_line and the gene lists (src/genes.rs:140-217), MethylationSite::from_methylome_file_line
(src/methylation_site.rs:146-362), is_in_gene / find_gene (:368-418) with the last_gene cache of Windows::extract
(src/windows.rs:303-338), place_in_windows (:423-490), Windows::new (src/windows.rs:28-44), Windows::save (:259-285) with
the directory tree of src/setup.rs:35-72, and the folds (src/windows.rs:94-128, src/pedigree.rs:165-166).  Python floats
are IEEE doubles: sequential +, -, / and * give the reference's bits.  Unsigned arithmetic wraps at 2^32 as the
reference's release build does.  No GPU, no product code — except pack_codes in packed_layout, which is the expectation
the issue names."""
import ctypes as C
from pathlib import Path

import numpy as np

SENSE, ANTISENSE, UNKNOWN = 0, 1, 2
M32 = 0xFFFFFFFF
REGIONS = ("upstream", "gene", "downstream")
HEADER = ("seqnames\tstart\tstrand\tcontext\tcounts.methylated\tcounts.total\tposteriorMax\tstatus\trc.meth.lvl\t"
          "context.trinucleotide\n")


class Args:  # arguments::Windows, the fields the extraction reads
    def __init__(self, cutoff=2048, step=5, size=5, absolute=False, cutoff_gene_length=False, flt=0.99):
        self.cutoff, self.size, self.absolute = cutoff, size, absolute
        self.step = size if step == 0 else step          # src/extract.rs:26-28
        self.cutoff_gene_length, self.flt = cutoff_gene_length, flt


# ---------------------------------------------------------------- parsing
def parse_u32(t, hi=M32):  # str::parse::<u32>: an optional '+', digits, no overflow
    d = t[1:] if t[:1] == "+" else t
    if not d or not all("0" <= ch <= "9" for ch in d) or int(d) > hi:
        return None
    return int(d)


def parse_f64(t):  # str::parse::<f64> on the spellings the tests use
    try:
        if not t or t != t.strip() or "_" in t:
            return None
        return float(t)
    except ValueError:
        return None


def chromosome(t):  # src/methylation_site.rs:55-68; Numbered(n) = n, M = 256, C = 257
    while t.startswith("chr"):
        t = t[3:]
    if t == "M":
        return 256
    if t == "C":
        return 257
    return parse_u32(t, 255)


def split2(s):  # s.split([' ', '\t'])
    return s.replace("\t", " ").split(" ")


def lines_of(text):  # BufRead::lines
    lines = text.split("\n")
    if lines and lines[-1] == "":
        lines.pop()
    return [l[:-1] if l.endswith("\r") else l for l in lines]


def gene_from_line(s):  # src/genes.rs:166-216
    f = split2(s)
    if len(f) != 6:
        return None
    ok = ("+", "-", "*")
    if f[5] in ok:       # first_format; a parse error here is final (:203: or_else only on None)
        strand, name = f[5], f[3]
    elif f[4] in ok:     # second_format
        strand, name = f[4], f[5]
    else:
        return None
    c, a, b = chromosome(f[0]), parse_u32(f[1]), parse_u32(f[2])
    if c is None or a is None or b is None:
        return None
    return dict(chromosome=c, start=a, end=b, strand=ok.index(strand), name=name)


def genome_of(text):  # src/extract.rs:30-67; list.sort_by is stable, like sorted()
    genome, genes = {}, []
    for line in lines_of(text):
        g = gene_from_line(line)
        if g is None:
            continue
        genes.append(g)
        c = genome.setdefault(g["chromosome"], dict(sense=[], antisense=[], combined=[]))
        c["combined"].append(g)
        if g["strand"] == SENSE:
            c["sense"].append(g)
        elif g["strand"] == ANTISENSE:
            c["antisense"].append(g)
    for c in genome.values():
        for k in c:
            c[k] = sorted(c[k], key=lambda g: g["start"])
    return genome, genes


def max_gene_length(genes, absolute):  # src/extract.rs:51-59
    return max((g["end"] - g["start"]) & M32 for g in genes) if absolute else 100


def site_from_line(s):  # src/methylation_site.rs:146-362
    tab = s.split("\t")

    def cg(chrom, s0, s1, strand, cm, ct, pm, st, ml):
        c, a = chromosome(tab[chrom]), parse_u32(tab[s0])
        if c is None or a is None:
            return None
        b = (a + 1) & M32 if s1 is None else parse_u32(tab[s1])
        post, lvl = parse_f64(tab[pm]), parse_f64(tab[ml])
        if b is None or parse_u32(tab[cm]) is None or parse_u32(tab[ct]) is None or post is None:
            return None
        if tab[st] == "" or lvl is None:
            return None
        status = {"M": 2, "I": 1}.get(tab[st][0], 0)
        return dict(chromosome=c, start=a, end=b, strand=SENSE if tab[strand] == "+" else ANTISENSE, posteriormax=post,
                    status=status, meth_lvl=lvl, original=s)

    if len(tab) in (9, 10) and tab[3] == "CG":
        r = cg(0, 1, None, 2, 4, 5, 6, 7, 8)
        if r:
            return r
    if len(tab) == 11 and tab[3] == "CG":
        r = cg(0, 1, 2, 5, 6, 7, 8, 9, 10)
        if r:
            return r
    ws = split2(s)
    if len(ws) == 4:   # chromatin state / bigwig
        c, a, b = chromosome(ws[0]), parse_u32(ws[1]), parse_u32(ws[2])
        if c is not None and a is not None and b is not None:
            return dict(chromosome=c, start=a, end=b, strand=UNKNOWN, posteriormax=0.0, status=0, meth_lvl=0.0, original=s)
    return None


# ---------------------------------------------------------------- gene choice
def strand_eq(a, b):  # src/genes.rs:88-96
    return not ((a == SENSE and b == ANTISENSE) or (a == ANTISENSE and b == SENSE))


def is_in_gene(site, gene, args):  # src/methylation_site.rs:368-378
    cutoff = (gene["end"] - gene["start"]) & M32 if args.cutoff_gene_length else args.cutoff
    return (site["chromosome"] == gene["chromosome"] and gene["start"] <= ((site["start"] + cutoff) & M32)
            and site["end"] <= ((gene["end"] + cutoff) & M32) and strand_eq(site["strand"], gene["strand"]))


def binary_search_by_key(lst, target, key):  # slice::binary_search_by, the `size / 2` form; Err(x) collapsed to x
    size, left, right = len(lst), 0, len(lst)
    while left < right:
        mid = left + size // 2
        k = key(lst[mid])
        if k == target:
            return mid
        if k < target:
            left = mid + 1
        else:
            right = mid
        size = right - left
    return left


def find_gene(site, genome, args):  # src/methylation_site.rs:385-418
    c = genome.get(site["chromosome"])
    if c is None:
        return None
    lst = c[("sense", "antisense", "combined")[site["strand"]]]
    if args.cutoff_gene_length:
        key = lambda g: (g["end"] + ((g["end"] - g["start"]) & M32)) & M32
    else:
        key = lambda g: (g["end"] + args.cutoff) & M32
    i = binary_search_by_key(lst, site["start"], key)
    if len(lst) < i + 1:
        return None
    return lst[i] if is_in_gene(site, lst[i], args) else None


def choose_genes(text, genome, args):
    """The loop of src/windows.rs:325-339 up to place_in_windows -> [(site, gene or None)] in file order"""
    out, last = [], None
    for line in lines_of(text)[1:]:
        site = site_from_line(line)
        if site is None:
            continue
        if last is None or not is_in_gene(site, last, args):
            last = find_gene(site, genome, args)
        site["index"] = len(out)   # its place among the file's sites
        out.append((site, last))
    return out


# ---------------------------------------------------------------- placement
def windows_new(args, mgl):  # src/windows.rs:28-44 -> (upstream, gene, downstream) counts
    ud = args.cutoff // args.step if args.absolute else 100 // args.step
    return ud, (mgl // args.step if args.absolute else 100 // args.step), ud


def place_in_windows(site, gene, args, counts):  # src/methylation_site.rs:423-490 -> (region index, [window, ..])
    E = 0.1
    location, cutoff, step, size = float(site["start"]), float(args.cutoff), float(args.step), float(args.size)
    start, end = float(gene["start"]), float(gene["end"])
    length = end - start
    anti = site["strand"] == ANTISENSE   # Unknown is placed as Sense
    offset = end - location if anti else location - start
    region = 0 if offset < 0.0 else (2 if offset > length else 1)
    if not anti:
        position = (location - start + cutoff, location - start, location - end)[region]
    else:
        position = (end - location + cutoff, end - location, start - location)[region]
    if not args.absolute:
        d = length if region == 1 else cutoff
        with np.errstate(all="ignore"):   # IEEE division: a gene of length 0 gives NaN or an infinity
            position = float(np.float64(position) / np.float64(d))
        position *= 100.0
    inside = []
    for i in range(counts[region]):
        lower = i * step - E
        upper = lower + size + E
        if position >= lower and position <= upper:
            inside.append(i)
    return region, inside


def extract(pairs, args, mgl):
    """Windows::extract's pushes: [region][window] -> [site, ..] in push order"""
    counts = windows_new(args, mgl)
    win = [[[] for _ in range(c)] for c in counts]
    for site, gene in pairs:
        if gene is None:
            continue
        region, inside = place_in_windows(site, gene, args, counts)
        for i in inside:
            win[region][i].append(site)
    return win


def flat(win):  # upstream, gene, downstream in one list (Windows::distribution's order)
    return win[0] + win[1] + win[2]


def code_of(site, flt):
    return site["status"] | (0x80 if site["posteriormax"] < flt else 0)


def soa(samples_pairs, args):
    """The arrays abn_windows_create takes for [pairs of sample 0, pairs of sample 1, ..]"""
    off = np.zeros(len(samples_pairs) + 1, dtype=np.int64)
    pos, gs, ge, fl, co, lv = [], [], [], [], [], []
    for s, pairs in enumerate(samples_pairs):
        off[s + 1] = off[s] + len(pairs)
        for site, gene in pairs:
            pos.append(site["start"])
            gs.append(gene["start"] if gene else 0)
            ge.append(gene["end"] if gene else 0)
            fl.append((1 if site["strand"] == ANTISENSE else 0) | (2 if gene else 0))
            co.append(code_of(site, args.flt))
            lv.append(site["meth_lvl"])
    return (off, np.array(pos, dtype=np.uint32), np.array(gs, dtype=np.uint32), np.array(ge, dtype=np.uint32),
            np.array(fl, dtype=np.uint8), np.array(co, dtype=np.uint8), np.array(lv, dtype=np.float64))


def folds(window, flt):
    """(level_sum, level_sum_kept, kept) of one window's sites: serial folds from 0.0 in push order"""
    all_, kept_sum, kept = 0.0, 0.0, 0
    for s in window:
        all_ = all_ + s["meth_lvl"]
        if s["posteriormax"] >= flt:
            kept_sum = kept_sum + s["meth_lvl"]
            kept += 1
    return all_, kept_sum, kept


def packed_layout_codes(abn, codes):
    """What layout_packed_call (host/pedigree_build.hpp) makes of codes[s][w] (u8 arrays: sample s, window w): window w's
    columns begin at a multiple of 256 sites; a ragged window has none; every other field is 3; at least one super-step
    per row.  -> (packed (n, stride) u8, begin, end, ragged)"""
    n, W = len(codes), len(codes[0])
    blocks, begin, end, ragged, off = [], [], [], [], 0
    for w in range(W):
        lens = {len(codes[s][w]) for s in range(n)}
        ragged.append(1 if len(lens) > 1 else 0)
        L = 0 if len(lens) > 1 else lens.pop()
        begin.append(4 * off)
        end.append(4 * off + L)
        if L:
            blocks.append(abn.pack_codes(np.array([codes[s][w] for s in range(n)], dtype=np.uint8)))
            off += blocks[-1].shape[1]
    packed = np.concatenate(blocks, axis=1) if blocks else np.full((n, 64), 0xFF, dtype=np.uint8)
    return packed, np.array(begin, dtype=np.int64), np.array(end, dtype=np.int64), np.array(ragged, dtype=np.int32)


def packed_layout(abn, wins, flt):
    """packed_layout_codes of the samples' windows: wins[s] = flat windows (site lists) of sample s"""
    return packed_layout_codes(abn, [[np.array([code_of(x, flt) for x in w], dtype=np.uint8) for w in ws] for ws in wins])


# ---------------------------------------------------------------- files
def fmt_f64(v):  # Rust's `{}`: shortest digits that round-trip, no exponent
    if v != v:
        return "NaN"
    if v in (float("inf"), float("-inf")):
        return "inf" if v > 0 else "-inf"
    return np.format_float_positional(v, unique=True, trim="-")


def save_tree(out_dir, args, mgl, nodes_text, edges_text, wins_by_name):
    """src/setup.rs:12-72 (directories for ceil(max / step) windows per region, nodelist with the sample paths rewritten,
    edgelist) and Windows::save (src/windows.rs:259-285) for every sample: wins_by_name[name] = [region][window] -> sites"""
    out_dir = Path(out_dir)
    for r, (side, mx) in enumerate(zip(REGIONS, (args.cutoff, mgl, args.cutoff))):
        mx = mx if args.absolute else 100
        for window in range(0, mx, args.step):
            d = out_dir / side / str(window)
            d.mkdir(parents=True, exist_ok=True)
            nodelist = ""
            for line in nodes_text.split("\n"):
                if line.startswith("/"):
                    old = line.split("\t")[0]
                    nodelist += line.replace(old, f"{out_dir}/{side}/{window}/{old.split('/')[-1]}")
                else:
                    nodelist += line
                nodelist += "\n"
            (d / "nodelist.txt").write_text(nodelist)
            (d / "edgelist.txt").write_text(edges_text)
    for name, win in wins_by_name.items():
        for r, side in enumerate(REGIONS):
            for i, sites in enumerate(win[r]):
                (out_dir / side / str(i * args.step) / name).write_text(HEADER + "\n".join(s["original"] for s in sites))


def side_files(names, wins_by_name):
    """src/extract.rs:100-151 with the methylomes in `names` order -> {file name: text}"""
    dist = {n: [len(w) for w in flat(wins_by_name[n])] for n in names}
    with np.errstate(all="ignore"):
        meth = {n: [np.float64(folds(w, 0.0)[0]) / np.float64(len(w)) for w in flat(wins_by_name[n])] for n in names}
    avg = [0.0] * len(dist[names[0]])
    for n in names:
        for i, v in enumerate(meth[n]):
            avg[i] += float(v) / float(len(names))
    out = {f"distribution_{n}": "".join(f"{c}\n" for c in dist[n]) for n in names}
    out["distributions.txt"] = "".join(n + ";" + "".join(f"{c};" for c in dist[n]) + "\n" for n in names)
    out["steady_state_methylation.txt"] = "".join(fmt_f64(v) + "\n" for v in avg)
    out["all_steady_state_methylation.txt"] = "".join(
        n + ";" + "".join(fmt_f64(float(v)) + ";" for v in meth[n]) + "\n" for n in names)
    return out


def site_line(chrom, pos, strand, status, post, level):
    return f"{chrom}\t{pos}\t{strand}\tCG\t3\t8\t{post!r}\t{status}\t{level!r}"


# ---------------------------------------------------------------- the host shims of host_capi.cpp
def hostlib():
    from alphabeta_rs_amd import build as B

    B.build_host()
    L = C.CDLL(str(B.PEDIGREE_LIB))
    ll, u32p, u8p = C.c_longlong, C.POINTER(C.c_uint32), C.POINTER(C.c_uint8)
    L.abh_annotation_lists.argtypes = [C.c_char_p, ll, C.c_char_p, ll, C.POINTER(ll)]
    L.abh_annotation_lists.restype = ll
    L.abh_choose_genes.argtypes = [C.c_char_p, ll, C.c_char_p, ll, C.c_uint, C.c_int, C.c_double, ll, u32p, u32p, u32p,
                                   u8p, u8p, C.POINTER(C.c_double)]
    L.abh_choose_genes.restype = ll
    L.abh_window_counts.argtypes = [C.c_uint, C.c_uint, C.c_uint, C.c_int, C.c_uint, C.POINTER(C.c_int)]
    L.abh_window_counts.restype = None
    return L


def host_choose_genes(L, annotation, methylome, args, cap=1 << 20):
    a, m = annotation.encode(), methylome.encode()
    pos, gs, ge = (np.zeros(cap, dtype=np.uint32) for _ in range(3))
    fl, co = np.zeros(cap, dtype=np.uint8), np.zeros(cap, dtype=np.uint8)
    lv = np.zeros(cap)
    u32p, u8p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint8)
    n = L.abh_choose_genes(a, len(a), m, len(m), args.cutoff, 1 if args.cutoff_gene_length else 0, args.flt, cap,
                           pos.ctypes.data_as(u32p), gs.ctypes.data_as(u32p), ge.ctypes.data_as(u32p),
                           fl.ctypes.data_as(u8p), co.ctypes.data_as(u8p), lv.ctypes.data_as(C.POINTER(C.c_double)))
    assert n >= 0
    return pos[:n], gs[:n], ge[:n], fl[:n], co[:n], lv[:n]
