"""The gene choice on the device (abn_genes_*, alphabeta_rs_amd/csrc/abn_genes.hpp) against the serial loop of the
reference as tests/_windows_model.py restates it: gene_start, gene_end and flags equal element for element; and the paths
built on it — Windows.from_sites and `metaprofile_alphabeta --genes device` — against the paths that choose on the host."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import _genes_model as G
import _windows_model as M

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden"


@pytest.fixture(scope="module")
def hand():
    return G.hand_cases()


def choose(abn, ctx, case):
    off, chrom, start, end, strand = case.want()[:5]
    genes = abn.Genes(ctx, G.gene_lists(case.genome))
    try:
        return ctx.choose_genes(genes, off, chrom, start, end, strand, cutoff=case.args.cutoff,
                                cutoff_gene_length=case.args.cutoff_gene_length)
    finally:
        genes.close()


def check(abn, ctx, case, label=""):
    gs, ge, fl, ms = choose(abn, ctx, case)
    want = case.want()
    assert np.array_equal(gs, want[5]) and np.array_equal(ge, want[6]) and np.array_equal(fl, want[7]), label
    return ms


def test_block_edges(abn, gpu_ctx, hand):
    case = hand["block_edges"]
    off, _, _, _, _, gs, _, fl = case.want()
    assert list(np.diff(off)) == [0, 1, 1023, 1024, 1025, 2049, 3000]
    s = off[6]
    assert list(gs[s + 1022:s + 1026]) == [10_000, 50_000, 90_000, 10_000] and fl[s + 2047] == 0 and fl[s + 2048] == 2
    assert np.all(gs[off[5]:off[6]] == 10_000)             # one gene over three blocks: two of them without a miss
    ms = check(abn, gpu_ctx, case)
    assert ms.shape == (3,) and np.all(ms > 0)


def test_sample_boundary(abn, gpu_ctx, hand):
    case = hand["sample_boundary"]
    off, _, _, _, _, gs, _, fl = case.want()
    assert len(set(np.diff(off))) == 3
    assert gs[off[1] - 1] == 1000 and gs[off[1]] == 2500 and fl[off[2]] == 0   # A kept to the end; C found; none
    check(abn, gpu_ctx, case)


def test_search(abn, gpu_ctx, hand):
    case = hand["search_lists"]
    genome = case.genome
    assert [len(genome[c]["sense"]) for c in range(1, 7)] == [1, 2, 3, 7, 8, 9] and 77 not in genome
    fl = case.want()[7]
    assert 0 < (fl & 2).sum() < len(fl)
    check(abn, gpu_ctx, case)


def test_strands(abn, gpu_ctx, hand):
    case = hand["strands"]
    off, _, _, _, strand, gs, _, _ = case.want()
    assert np.all(gs[400:600:2] == 1000) and np.all(gs[401:600:2] == 1200)            # every site a miss
    o = off[1]
    assert list(gs[o:o + 4]) == [1000] * 4 and list(strand[o:o + 3]) == [2, 0, 1]     # the `*` gene kept by + and -
    check(abn, gpu_ctx, case)


def test_wrapping_arithmetic(abn, gpu_ctx, hand):
    for name in ("wrap_cutoff", "wrap_gene_length"):
        fl = hand[name].want()[7]
        assert 0 < (fl & 2).sum() < len(fl)
        check(abn, gpu_ctx, hand[name], name)


def test_unsorted_input(abn, gpu_ctx):
    """positions in random order, three chromosomes interleaved, 2500 sites: three blocks"""
    rng = np.random.default_rng(9)
    ann = "".join(G.gene_line(c, int(a), int(a) + int(l), "+-"[int(k)]) for c, a, l, k in
                  zip(rng.integers(1, 4, size=60), rng.integers(0, 50_000, size=60), rng.integers(10, 4000, size=60),
                      rng.integers(0, 2, size=60)))
    rows = [G.cg(int(c), int(p), "+-"[int(k)]) for c, p, k in
            zip(rng.integers(1, 4, size=2500), rng.integers(0, 56_000, size=2500), rng.integers(0, 2, size=2500))]
    case = G.Case(ann, [G.text(rows)], cutoff=100)
    fl = case.want()[7]
    assert 0 < (fl & 2).sum() < len(fl)
    check(abn, gpu_ctx, case)


class DeviceArrays:
    """device buffers from the HIP runtime the product library already holds (as tests/test_pairwise_windows.py)"""

    def __init__(self):
        hip = C.CDLL("libamdhip64.so")
        hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        hip.hipFree.argtypes = [C.c_void_p]
        self.hip, self.held = hip, []

    def up(self, a):
        p = C.c_void_p()
        assert self.hip.hipMalloc(C.byref(p), max(a.nbytes, 16)) == 0
        self.held.append(p)
        if a.nbytes:
            assert self.hip.hipMemcpy(p, a.ctypes.data, a.nbytes, 1) == 0
        return p.value

    def down(self, ptr, a):
        if a.nbytes:
            assert self.hip.hipMemcpy(a.ctypes.data, C.c_void_p(ptr), a.nbytes, 2) == 0
        return a

    def free(self):
        for p in self.held:
            self.hip.hipFree(p)
        self.held = []


def test_seeded_slice_host_and_device_entries_twice(abn, gpu_ctx):
    """200 seeded cases of at most 3000 sites and 80 genes through abn_genes_choose and abn_genes_choose_dev, each twice:
    equal to the model, and byte-identical from run to run."""
    dev = DeviceArrays()
    try:
        for seed in range(1000, 1200):
            case = G.random_case(seed, 3000, 80)
            off, chrom, start, end, strand, gs, ge, fl = case.want()
            genes = abn.Genes(gpu_ctx, G.gene_lists(case.genome))
            kw = dict(cutoff=case.args.cutoff, cutoff_gene_length=case.args.cutoff_gene_length)
            S = int(off[-1])
            ptrs = [dev.up(a) for a in (chrom, start, end, strand)]
            for run in range(2):
                got = gpu_ctx.choose_genes(genes, off, chrom, start, end, strand, **kw)
                assert got[0].tobytes() == gs.tobytes() and got[1].tobytes() == ge.tobytes() and got[2].tobytes() == fl.tobytes(), seed
                outs = [dev.up(np.full(S, 0xAB, dtype=t)) for t in (np.uint32, np.uint32, np.uint8)]
                gpu_ctx.choose_genes_dev(genes, off, *ptrs, *outs, **kw)
                back = [dev.down(p, np.zeros(S, dtype=t)) for p, t in zip(outs, (np.uint32, np.uint32, np.uint8))]
                assert back[0].tobytes() == gs.tobytes() and back[1].tobytes() == ge.tobytes() and back[2].tobytes() == fl.tobytes(), seed
            genes.close()
            dev.free()
    finally:
        dev.free()


def window_case():
    """four samples on the same coordinates over three genes of both strands, statuses and posteriors their own: no
    window is ragged, and the pairwise scan has something to count"""
    rng = np.random.default_rng(12)
    ann = G.gene_line(1, 5000, 9000, "+") + G.gene_line(1, 20_000, 26_000, "-") + G.gene_line(2, 3000, 4000, "+")
    where = ([(1, int(p), "+") for p in np.sort(rng.integers(2500, 11_500, size=900))] +
             [(1, int(p), "-") for p in np.sort(rng.integers(17_500, 28_500, size=900))] +
             [(2, int(p), "+-"[i % 2]) for i, p in enumerate(np.sort(rng.integers(500, 6500, size=700)))])
    texts = []
    for k in range(4):
        texts.append(G.text(M.site_line(c, p, s, "UIM"[int(rng.integers(3))], [0.9999, 0.7][int(rng.integers(8) == 0)],
                                        round(float(rng.random()), 4)) for c, p, s in where))
    return ann, texts


def test_windows_from_sites_equals_windows_fed_with_the_host_choice(abn, gpu_ctx):
    ann, texts = window_case()
    args = M.Args(cutoff=2048, step=5, size=5, absolute=False)
    genome, genes = M.genome_of(ann)
    pairs = [M.choose_genes(t, genome, args) for t in texts]
    off, pos, gs, ge, fl, co, lv = M.soa(pairs, args)
    counts = M.windows_new(args, 100)
    kw = dict(cutoff=args.cutoff, step=args.step, size=args.size, absolute=args.absolute, counts=counts)
    sites = [s for p in pairs for s, _ in p]
    col = lambda k, t: np.array([s[k] for s in sites], dtype=t)
    g = abn.Genes(gpu_ctx, G.gene_lists(genome))
    a = abn.Windows(gpu_ctx, off, pos, gs, ge, fl, co, lv, **kw)
    b = abn.Windows.from_sites(gpu_ctx, g, off, col("chromosome", np.int32), col("start", np.uint32), col("end", np.uint32),
                               col("strand", np.uint8), co, lv, **kw)
    try:
        assert (b.W, b.row_stride, b.n_sites, b.n_samples) == (a.W, a.row_stride, a.n_sites, a.n_samples)
        assert a.stats()[0].sum() > 4 * 1500 and not a.layout()[2].any()
        assert np.array_equal(a.packed(), b.packed())
        for x, y in zip(a.stats() + a.layout(), b.stats() + b.layout()):
            assert x.dtype == y.dtype and x.tobytes() == y.tobytes()
        for x, y in zip(a.pairwise(), b.pairwise()):
            assert x.tobytes() == y.tobytes()
        assert a.pairwise()[1].any()
    finally:
        a.close()
        b.close()
        g.close()


def test_metaprofile_genes_device_equals_genes_host(abn, tmp_path):
    """the fixture of tests/test_windows_gpu.py::test_metaprofile_in_memory_equals_the_directory_path (synthetic methylomes
    of the bundled 4-sample pedigree over the first genes of the annotation): every output file of --genes device is the
    file of --genes host, under --parse host and --parse device"""
    from alphabeta_rs_amd import build as B

    B.build_host()
    genome, genes = M.genome_of((GOLDEN / "annotation.txt").read_text())
    rng = np.random.default_rng(8)
    where = []
    for g in sorted(genes, key=lambda g: (g["chromosome"], g["start"]))[:3]:
        where += [(g, int(p)) for p in sorted(rng.integers(g["start"] - 2100, g["end"] + 2100, size=1000))]
    names = ["G0.txt", "G1_2.txt", "G4_2.txt", "G4_8.txt"]
    meth = tmp_path / "methylome"
    meth.mkdir()
    status = rng.choice([0, 2], size=len(where), p=[0.6, 0.4])
    for k, name in enumerate(names):
        if k:
            flip = rng.random(len(where)) < 0.04 * k
            status = np.where(flip, rng.integers(0, 3, size=len(where)), status)
        rows = [(g["chromosome"], p, "+-*"[g["strand"]].replace("*", "+"), "UIM"[int(s)], [0.9999, 0.7][int(rng.integers(10) == 0)],
                 round(float(0.05 + 0.45 * s + 0.04 * rng.random()), 4)) for (g, p), s in zip(where, status)]
        (meth / name).write_text(M.HEADER + "".join(M.site_line(*r) + "\n" for r in rows))
    nodes = "filename\tnode\tgen\tmeth\n" + "".join(
        f"{meth}/{f}\t{node}\t{gen}\t{m}\n" for f, node, gen, m in
        [("G0.txt", "0_0", 0, "Y"), ("G1_2.txt", "1_2", 1, "Y"), ("G1_8.txt", "1_8", 1, "N"), ("G2_2.txt", "2_2", 2, "N"),
         ("G2_8.txt", "2_8", 2, "N")]) + "-\t3_2\t3\tN\n-\t3_8\t3\tN\n" + f"{meth}/G4_2.txt\t4_2\t4\tY\n{meth}/G4_8.txt\t4_8\t4\tY\n"
    (tmp_path / "nodelist.fn").write_text(nodes)
    (tmp_path / "edgelist.fn").write_text((GOLDEN / "data" / "edgelist.txt").read_text())
    files = {}
    for parse in ("host", "device"):
        for where_genes in ("host", "device"):
            out = tmp_path / f"out_{parse}_{where_genes}"
            out.mkdir()
            r = subprocess.run([str(B.META_CLI), "-o", str(out), "--methylome", str(meth), "--genome",
                                str(GOLDEN / "annotation.txt"), "--nodes", str(tmp_path / "nodelist.fn"), "--edges",
                                str(tmp_path / "edgelist.fn"), "--iterations", "10", "--seed", "77", "-s", "5", "-w", "5",
                                "-c", "2048", "--parse", parse, "--genes", where_genes],
                               capture_output=True, text=True, timeout=300)
            assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
            files[parse, where_genes] = {p.name: p.read_bytes() for p in sorted(out.iterdir())}
        a, b = files[parse, "host"], files[parse, "device"]
        assert sorted(a) == sorted(b) and len(a) >= 9 and len(a["results.txt"].splitlines()) > 50
        for name in a:
            assert a[name] == b[name], (parse, name)
    r = subprocess.run([str(B.META_CLI), "-o", str(tmp_path), "--genes", "gpu"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--genes expects host or device" in r.stderr


def test_bad_arguments_are_status_codes_and_launch_nothing(abn, gpu_ctx):
    L = gpu_ctx._L
    i32, i64, u32, u8 = (lambda *v: np.array(v, dtype=np.int32)), (lambda *v: np.array(v, dtype=np.int64)), \
        (lambda *v: np.array(v, dtype=np.uint32)), (lambda *v: np.array(v, dtype=np.uint8))
    p = lambda a: a.ctypes.data_as(C.c_void_p)

    def create(n, chrom, kind, off, start=u32(1, 5), end=u32(9, 9), strand=u8(0, 0)):
        h = C.c_void_p()
        rc = L.abn_genes_create(gpu_ctx._h, n, *(None if a is None else C.cast(p(a), t) for a, t in
                                                  zip((chrom, kind, off, start, end, strand), L.abn_genes_create.argtypes[2:8])),
                                C.byref(h))
        if rc == 0:
            L.abn_genes_destroy(h)
        return rc

    assert create(1, i32(1), i32(0), i64(0, 2)) == 0
    assert create(0, None, None, i64(0), None, None, None) == 0          # an empty annotation is an annotation
    for bad in ((1, None, i32(0), i64(0, 2)), (1, i32(1), i32(0), None), (1, i32(1), i32(0), i64(0, 2), None),
                (1, i32(258), i32(0), i64(0, 2)), (1, i32(-1), i32(0), i64(0, 2)), (1, i32(1), i32(3), i64(0, 2)),
                (2, i32(1, 1), i32(0, 0), i64(0, 1, 2)), (1, i32(1), i32(0), i64(1, 2)), (2, i32(1, 2), i32(0, 0), i64(0, 2, 1)),
                (-1, i32(1), i32(0), i64(0, 2))):
        assert create(*bad) == 1, bad
    assert L.abn_genes_create(None, 0, None, None, None, None, None, None, None) == 1
    genes = abn.Genes(gpu_ctx, [(1, 0, [10], [90], [0])])
    try:
        ok = dict(cutoff=5)
        chrom, start, end, strand = i32(1, 1, 1), u32(20, 30, 500), u32(21, 31, 501), u8(0, 0, 0)
        gs, ge, fl, _ = gpu_ctx.choose_genes(genes, [0, 3], chrom, start, end, strand, **ok)
        assert list(gs) == [10, 10, 0] and list(ge) == [90, 90, 0] and list(fl) == [2, 2, 0]
        assert [len(a) for a in gpu_ctx.choose_genes(genes, [0, 0, 0], chrom[:0], start[:0], end[:0], strand[:0], **ok)[:3]] == [0, 0, 0]
        rule = abn.GeneRule(5, 0)
        outs = [np.full(3, 0xAB, dtype=np.uint32), np.full(3, 0xAB, dtype=np.uint32), np.full(3, 0xAB, dtype=np.uint8)]

        def call(off, c=chrom, d=strand, r=rule, n=1, h=genes._h):
            a = L.abn_genes_choose.argtypes
            return L.abn_genes_choose(h, C.byref(r) if r else None, n, None if off is None else C.cast(p(off), a[3]),
                                      C.cast(p(c), a[4]), C.cast(p(start), a[5]), C.cast(p(end), a[6]), C.cast(p(d), a[7]),
                                      C.cast(p(outs[0]), a[8]), C.cast(p(outs[1]), a[9]), C.cast(p(outs[2]), a[10]), None)

        assert call(i64(0, 3)) == 0 and list(outs[0]) == [10, 10, 0]
        for o in outs:
            o.fill(0xAB)
        for rc in (call(None), call(i64(0, 3), r=None), call(i64(0, 3), n=0), call(i64(1, 3)), call(i64(0, 3, 2), n=2),
                   call(i64(0, 3), c=i32(1, 258, 1)), call(i64(0, 3), c=i32(1, 1, -1)), call(i64(0, 3), d=u8(0, 3, 0)),
                   call(i64(0, 3), h=None)):
            assert rc == 1
        assert all(np.all(o == 0xAB) for o in outs)                    # nothing was written: no kernel ran
        # the device form finds a bad chromosome in its kernels; Windows.from_sites checks on the host, like Windows
        dev = DeviceArrays()
        try:
            ptrs = [dev.up(a) for a in (i32(1, 300, 1), start, end, strand)] + [dev.up(o) for o in outs]
            with pytest.raises(abn.AbnError) as err:
                gpu_ctx.choose_genes_dev(genes, [0, 3], *ptrs, **ok)
            assert err.value.status == 1
        finally:
            dev.free()
        kw = dict(cutoff=10, size=5, absolute=False)
        z8, lv = np.zeros(3, dtype=np.uint8), np.zeros(3)
        for off, c, step, counts in (([0, 3], i32(1, 258, 1), 5, (1, 1, 1)), ([0, 3], chrom, 0, (1, 1, 1)),
                                     ([1, 3], chrom, 5, (1, 1, 1)), ([0, 3], chrom, 5, (1, -1, 1))):
            with pytest.raises(abn.AbnError) as err:
                abn.Windows.from_sites(gpu_ctx, genes, off, c, start, end, strand, z8, lv, step=step, counts=counts, **kw)
            assert err.value.status == 1
    finally:
        genes.close()
