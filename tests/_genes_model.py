"""Cases and helpers of the gene-choice tests (tests/test_genes_cpu.py, tests/test_genes_gpu.py).  A case is an annotation
text, methylome texts (one per sample) and the arguments; the expectation is always _windows_model.choose_genes, the
restatement of the serial loop of src/windows.rs:325-338.  No product code here except the bindings of the host shim."""
import ctypes as C

import numpy as np

import _windows_model as M

BLOCK = 1024   # kGeneBlockSites


class Case:
    def __init__(self, annotation, texts, cutoff=2048, cutoff_gene_length=False):
        self.annotation, self.texts = annotation, list(texts)
        self.args = M.Args(cutoff=cutoff, cutoff_gene_length=cutoff_gene_length)
        self._want = None

    @property
    def genome(self):
        return M.genome_of(self.annotation)[0]

    def want(self):
        """(site_offset, chromosome, start, end, strand, gene_start, gene_end, flags) of the model, computed once"""
        if self._want is None:
            genome = self.genome
            pairs = [M.choose_genes(t, genome, self.args) for t in self.texts]
            off, _, gs, ge, fl, _, _ = M.soa(pairs, self.args)
            sites = [s for p in pairs for s, _ in p]
            col = lambda k, t: np.array([s[k] for s in sites], dtype=t)
            self._want = (off, col("chromosome", np.int32), col("start", np.uint32), col("end", np.uint32),
                          col("strand", np.uint8), gs, ge, fl)
        return self._want


def gene_line(chrom, start, end, strand, name="g"):
    return f"{chrom}\t{start}\t{end}\t{name}\tx\t{strand}\n"


def cg(chrom, pos, strand):
    return M.site_line(chrom, pos, strand, "M", 0.9999, 0.5)


def region(chrom, a, b):   # a 4-field row: Unknown strand
    return f"{chrom}\t{a}\t{b}\tstate"


def text(lines):
    return M.HEADER + "".join(l + "\n" for l in lines)


def gene_lists(genome):
    """the lists of a model genome as Genes(ctx, lists) takes them"""
    out = []
    for chrom in sorted(genome):
        for kind, key in enumerate(("sense", "antisense", "combined")):
            lst = genome[chrom][key]
            if lst:
                out.append((chrom, kind, [g["start"] for g in lst], [g["end"] for g in lst], [g["strand"] for g in lst]))
    return out


# ---------------------------------------------------------------- hand-made cases
def block_edges():
    """Samples of 0, 1, 1023, 1024, 1025 and 2049 sites inside one gene (no miss behind the first site: the blocks behind
    the first have entry END and pass the carry through), and one of 3000 sites with a miss exactly at the last site of
    block 0 (another gene), at the first site of block 1 (a third), a site without a gene as the last site of block 1, and
    the run of the first gene picked up again behind each."""
    ann = gene_line(1, 10_000, 20_000, "+") + gene_line(1, 50_000, 51_000, "+") + gene_line(1, 90_000, 91_000, "+")
    inside = lambda n: text(cg(1, 10_000 + (i * 7) % 9000, "+") for i in range(n))
    rows = [cg(1, 10_000 + (i * 7) % 9000, "+") for i in range(3000)]
    rows[BLOCK - 1] = cg(1, 50_500, "+")
    rows[BLOCK] = cg(1, 90_500, "+")
    rows[2 * BLOCK - 1] = cg(1, 500_000, "+")
    return Case(ann, [inside(n) for n in (0, 1, 1023, 1024, 1025, 2049)] + [text(rows)], cutoff=100)


def sample_boundary():
    """Genes A (1000, 9000), B (2000, 3000), C (2500, 8000), cutoff 0: a site at 1500 finds A and a site at 5000 keeps it,
    while find_gene of 5000 alone probes B, then C, and answers C.  Sample 1 ends at 5000 holding A; sample 2 begins at
    5000 and must start from nothing: C.  Sample 3 begins outside every gene."""
    ann = gene_line(1, 1000, 9000, "+", "A") + gene_line(1, 2000, 3000, "+", "B") + gene_line(1, 2500, 8000, "+", "C")
    s1 = [cg(1, 1500, "+")] + [cg(1, 5000 + i % 50, "+") for i in range(1500)]
    s2 = [cg(1, 5000 + i % 50, "+") for i in range(700)] + [cg(1, 1500, "+"), cg(1, 5000, "+")]
    s3 = [cg(1, 20_000, "+")] + [cg(1, 5000, "+")] * 2100
    return Case(ann, [text(s1), text(s2), text(s3)], cutoff=0)


def search_lists():
    """Chromosomes 1..6 with lists of 1, 2, 3, 7, 8, 9 genes — nested, overlapping, with equal search keys (equal ends), so
    the answer depends on the probe sequence; chromosome 77 has no list; positions from left of every key to right of
    every key, every chromosome's sites interleaved with the others'."""
    rng = np.random.default_rng(41)
    ann, rows = "", []
    for chrom, n in zip(range(1, 7), (1, 2, 3, 7, 8, 9)):
        ends = rng.choice([3000, 4000, 5000, 6000], size=n)          # few distinct ends: equal keys
        for e in ends:
            ann += gene_line(chrom, int(rng.integers(500, int(e))), int(e), "+")
        ann += gene_line(chrom, 100, 9000, "-")                        # the antisense list: one gene
    for p in range(0, 9200, 37):
        for chrom in (1, 2, 3, 4, 5, 6, 77):
            rows.append(cg(chrom, p, "+"))
    order = rng.permutation(len(rows))
    return Case(ann, [text(rows), text([rows[i] for i in order])], cutoff=100)


def strands():
    """Alternating + / - sites (every site is a miss); Unknown-strand rows against the combined list; a `*` gene that an
    Unknown row finds and that the following + and - sites keep — alone they would search lists that do not hold it."""
    ann = (gene_line(2, 1000, 3000, "+") + gene_line(2, 1200, 3200, "-") + gene_line(3, 1000, 2000, "*") +
           gene_line(3, 5000, 6000, "+"))
    alt = [cg(2, 900 + 3 * i, "+-"[i % 2]) for i in range(1100)]
    unk = [region(3, 1500, 1501), cg(3, 1600, "+"), cg(3, 1700, "-"), cg(3, 1800, "+"), cg(3, 5500, "-"), cg(3, 5500, "+"),
           region(3, 5400, 5600), region(2, 1100, 1150), cg(3, 1600, "+"), region(3, 900, 2050), region(3, 800, 2200)]
    return Case(ann, [text(alt), text(unk), text(alt + unk * 30)], cutoff=100)


def wraps():
    """start + cutoff and end + cutoff beyond 2^32 (u32 arithmetic wraps), and with cutoff_gene_length a gene whose end is
    below its start: a `cutoff` of end - start mod 2^32."""
    top = 2 ** 32
    ann = gene_line(4, top - 1000, top - 10, "+") + gene_line(4, top - 300, top - 200, "+") + gene_line(4, 5, 40, "+")
    rows = [cg(4, p, "+") for p in (top - 1200, top - 1001, top - 1000, top - 500, top - 250, top - 101, top - 100,
                                      top - 11, top - 2, 0, 5, 39, 60, 139, 141, top - 2, 30)]
    a = Case(ann, [text(rows * 70)], cutoff=100)
    ann2 = gene_line(5, 3000, 1000, "+") + gene_line(5, 2000, 2600, "+") + gene_line(5, 100, 900, "-")
    rows2 = [cg(5, p, "+-"[(p // 7) % 2]) for p in range(0, 6000, 13)] + [cg(5, top - 5, "+"), cg(5, 1001, "+")]
    b = Case(ann2, [text(rows2 * 3)], cutoff=0, cutoff_gene_length=True)
    return [a, b]


def random_case(seed, max_sites, max_genes):
    """A seeded case: 1..3 samples; sorted or unsorted positions; alternating, random or single strands; some Unknown rows;
    nested, overlapping and equal-keyed genes of every strand; cutoff 0, 100 or 2048, sometimes cutoff_gene_length.  Most
    cases are small; the site counts reach past the block edges."""
    rng = np.random.default_rng(seed)
    span = int(rng.choice([2_000, 20_000, 200_000]))
    chroms = [int(c) for c in rng.choice([1, 2, 3, 256, 257], size=int(rng.integers(1, 4)), replace=False)]
    names = {256: "M", 257: "C"}
    ann = ""
    for _ in range(int(rng.integers(0, max_genes + 1))):
        a = int(rng.integers(0, span))
        length = int(rng.choice([0, 5, 50, 500, 5000])) + int(rng.integers(0, 50))
        b = a + length if rng.random() < 0.8 else int(rng.choice([span // 2, span // 3, span]))   # shared ends
        c = chroms[int(rng.integers(len(chroms)))]
        ann += gene_line(names.get(c, c), a, b, "+-*"[int(rng.choice(3, p=[.45, .45, .1]))])
    cutoff = int(rng.choice([0, 100, 2048]))
    texts = []
    for _ in range(int(rng.integers(1, 4))):
        top = int(rng.choice([40, min(1100, max_sites), max_sites], p=[.6, .25, .15]))
        n = int(rng.integers(0, top + 1))
        pos = rng.integers(0, span + 3000, size=n)
        if rng.random() < 0.7:
            pos = np.sort(pos)
        mode = int(rng.integers(3))
        rows = []
        for i, p in enumerate(pos):
            c = chroms[0] if rng.random() < 0.9 else chroms[int(rng.integers(len(chroms)))]
            c = names.get(c, c)
            if rng.random() < 0.05:
                rows.append(region(c, int(p), int(p) + int(rng.integers(0, 300))))
            else:
                rows.append(cg(c, int(p), "+-"[i % 2] if mode == 0 else ("+-"[int(rng.integers(2))] if mode == 1 else "+")))
        texts.append(text(rows))
    return Case(ann, texts, cutoff=cutoff, cutoff_gene_length=bool(rng.random() < 0.2))


def hand_cases():
    return {"block_edges": block_edges(), "sample_boundary": sample_boundary(), "search_lists": search_lists(),
            "strands": strands(), "wrap_cutoff": wraps()[0], "wrap_gene_length": wraps()[1]}


# ---------------------------------------------------------------- the host shim of host_capi.cpp
def hostlib():
    L = M.hostlib()
    ll, u32p, u8p = C.c_longlong, C.POINTER(C.c_uint32), C.POINTER(C.c_uint8)
    L.abh_choose_genes_blocked.argtypes = [C.c_char_p, ll, C.POINTER(C.c_char_p), C.POINTER(ll), C.c_int, C.c_uint,
                                           C.c_int, C.c_int, ll, C.POINTER(ll), u32p, u32p, u8p]
    L.abh_choose_genes_blocked.restype = ll
    return L


def host_choose_blocked(L, case, block_sites):
    """abh_choose_genes_blocked -> (site_offset, gene_start, gene_end, flags)"""
    a = case.annotation.encode()
    texts = [t.encode() for t in case.texts]
    n = len(texts)
    cap = sum(t.count(b"\n") for t in texts) + 1
    arr = (C.c_char_p * n)(*texts)
    lens = (C.c_longlong * n)(*map(len, texts))
    off = (C.c_longlong * (n + 1))()
    gs, ge, fl = np.zeros(cap, dtype=np.uint32), np.zeros(cap, dtype=np.uint32), np.zeros(cap, dtype=np.uint8)
    u32p, u8p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint8)
    S = L.abh_choose_genes_blocked(a, len(a), arr, lens, n, case.args.cutoff, 1 if case.args.cutoff_gene_length else 0,
                                   block_sites, cap, off, gs.ctypes.data_as(u32p), ge.ctypes.data_as(u32p),
                                   fl.ctypes.data_as(u8p))
    assert S >= 0, S
    return np.array(list(off), dtype=np.int64), gs[:S], ge[:S], fl[:S]
