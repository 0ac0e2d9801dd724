"""Methylomes aligned by position on the device (abn_sites_common, abn_windows_create_aligned, abn_codes_create_aligned;
alphabeta_rs_amd/csrc/abn_sites_common.hpp).  The oracle is what the project already has, fed pre-filtered input: the common
set is computed here from sets of key tuples, the rows outside it are removed in Python, and the aligned result must be
byte-identical to the existing path on what is left."""
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

import _codes_model as K
import _common_model as X
import _genes_model as G
import _parse_model as P
import _windows_model as M
from test_sites_resident_gpu import Deferring, decide, slabs

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden"
FLT = K.FILTER
INVALID = 1  # ABN_ERR_INVALID_ARG
COMMON_COUNTS = (0, 1, 63, 64, 65, 255, 256, 257, 1025)


@pytest.fixture(scope="module")
def L():
    return P.hostlib()


# ---------------------------------------------------------------- the step alone
def device(ctx, samples):
    """Context.common_sites -> ("ok", keep per sample, n_common)"""
    off, chrom, start, end, strand = X.concat(samples)
    keep, n = ctx.common_sites(off, chrom, start, end, strand)
    assert keep.dtype == np.uint8 and keep.shape == (int(off[-1]),)
    return ("ok", [keep[off[s]:off[s + 1]] for s in range(len(samples))], n)


def assert_same(got, want, name):
    assert want[0] == "ok" and got[2] == want[2], (name, got[2], want[1:])
    for g, w in zip(got[1], want[1]):
        assert g.tobytes() == w.tobytes(), name


def test_common_sites_against_the_set_intersection(gpu_ctx):
    rng = np.random.default_rng(20261019)
    first = last = whole = 0
    for n_common in COMMON_COUNTS:
        for n_samples in (1, 2, 3, 5):
            extra = (0, 7, 40)[(n_common + n_samples) % 3]
            samples = X.make_case(rng, n_samples, n_common, extra, chrom_order=((1, 10, 2), (2, 1, 257, 256))[n_samples % 2],
                                  lonely=(None, 30)[n_common % 2], drop_first=n_common % 3 == 0, drop_last=n_common % 3 == 1)
            got = device(gpu_ctx, samples)
            assert_same(got, X.model(samples), (n_common, n_samples))
            assert got[2] == n_common
            a, b, c = X.coverage(samples, got[1])
            first, last, whole = first + a, last + b, whole + c
    assert first >= 5 and last >= 5 and whole >= 5, (first, last, whole)


def test_common_sites_edges(gpu_ctx):
    key = lambda i, c=1: (c, 10 + i, 11 + i, i % 3)
    big = [key(i) for i in range(3000)]
    # the shortest sample (the one whose sites are looked up) changes chromosome exactly at a workgroup's edge: site 256
    edge = [key(i, 1) for i in range(256)] + [key(i, 2) for i in range(300)]
    other = [key(i, 1) for i in range(0, 400, 2)] + [key(i, 2) for i in range(1, 500)]
    for name, samples, n_common in (
            ("one sample", [big[:300]], 300),
            ("one empty sample", [[]], 0),
            ("an empty sample among others", [big[:10], [], big[:10]], 0),
            ("1 and 3000, common", [[big[1234]], big], 1),
            ("3000 and 1, the last site", [big, [big[2999]]], 1),
            ("1 and 3000, not common", [[(1, 5, 5, 0)], big], 0),
            ("all common", [big[:257], big[:257], big[:257]], 257),
            ("none common", [big[:100], big[100:200]], 0),
            ("a run boundary on a workgroup edge", [edge, other + [key(0, 3)]], 128 + 299),
            ("a chromosome missing from one", [big[:50] + [key(i, 2) for i in range(9)], big[:50]], 50),
            ("only end differs", [[(1, 5, 6, 0), (1, 5, 7, 0)], [(1, 5, 7, 0)]], 1),
            ("only strand differs", [[(1, 5, 6, 0), (1, 5, 6, 2)], [(1, 5, 6, 1), (1, 5, 6, 2)]], 1),
            ("runs 1, 10, 2 with organelles", [[key(0, 1), key(0, 10), key(0, 2), key(0, 256), key(0, 257)],
                                                [key(0, 1), key(1, 10), key(0, 2), key(0, 257)]], 3)):
        got = device(gpu_ctx, samples)
        assert_same(got, X.model(samples), name)
        assert got[2] == n_common, name


def test_common_sites_refusals(abn, gpu_ctx):
    rng = np.random.default_rng(7)
    kinds = {X.SPLIT: 0, X.NOT_ASCENDING: 0, X.NOT_COORDERED: 0}
    for name, samples, kind in X.refusal_cases(rng):
        want = X.model(samples)
        assert want[:2] == ("refused", kind), (name, want)
        with pytest.raises(abn.AbnError) as e:
            device(gpu_ctx, samples)
        assert e.value.status == INVALID, name
        assert f"sample {want[2]}, site {want[3]}: {X.WORDS[kind]}" in str(e.value), (name, str(e.value), want)
        kinds[kind] += 1
    assert min(kinds.values()) >= 3, kinds
    with pytest.raises(abn.AbnError) as e:                                          # no index into the table of runs
        device(gpu_ctx, [[(1, 1, 1, 0), (258, 1, 1, 0)]])
    assert e.value.status == INVALID and "sample 0, site 1" in str(e.value)
    lib = gpu_ctx._L                                                               # the argument checks of the siblings
    off = np.array([0, 0], dtype=np.int64)
    n = np.zeros(1, dtype=np.int64)
    i64 = lambda a: a.ctypes.data_as(lib.abn_sites_common.argtypes[2])
    assert lib.abn_sites_common(None, 1, i64(off), None, None, None, None, None, i64(n)) == INVALID
    assert lib.abn_sites_common(gpu_ctx._h, 0, i64(off), None, None, None, None, None, i64(n)) == INVALID
    assert lib.abn_sites_common(gpu_ctx._h, 1, None, None, None, None, None, None, i64(n)) == INVALID
    assert lib.abn_sites_common(gpu_ctx._h, 1, i64(off), None, None, None, None, None, None) == INVALID
    assert lib.abn_sites_common(gpu_ctx._h, 1, i64(np.array([0, 3], dtype=np.int64)), None, None, None, None, None, i64(n)) == INVALID
    assert lib.abn_sites_common(gpu_ctx._h, 1, i64(off), None, None, None, None, None, i64(n)) == 0 and n[0] == 0


# ---------------------------------------------------------------- samples that share most of their sites
def keys_of(sites):
    return list(zip(*(sites[k].tolist() for k in ("chromosome", "start", "end", "strand"))))


def common_masks(fetched):
    """from the fetched (or merged) records of every sample: the boolean mask of its common sites"""
    keys = [keys_of(f) for f in fetched]
    want = X.model(keys)
    assert want[0] == "ok", want
    return [k.astype(bool) for k in want[1]], want[2]


def thin(rng, rows, lose):
    """the rows of a sample without `lose` of them"""
    gone = set(rng.choice(len(rows), size=lose, replace=False).tolist())
    return [r for i, r in enumerate(rows) if i not in gone]


def mark(d):
    """rows the device defers at the edges of its first slabs and in the middle: the common step sees merged records of
    both sources"""
    for chunk in (0, 1, 2):
        d.mark_chunk_edges(chunk)
    n = len(d.lines)
    if n > 40:
        d.mark(n // 2), d.mark(n // 2 + 1)
    return d


def test_windows_aligned_equals_from_sites_on_the_filtered_arrays(abn, gpu_ctx, L):
    rng = np.random.default_rng(11)
    ann = G.gene_line(1, 4000, 9000, "+") + G.gene_line(1, 20000, 24000, "-") + G.gene_line(2, 3000, 8000, "+")
    genome, _ = M.genome_of(ann)
    universe = []
    for chrom, lo, hi in ((1, 1500, 11500), (1, 17500, 26500), (2, 500, 10500)):
        for p in sorted(set(rng.integers(lo, hi, size=420).tolist())):
            universe.append((chrom, p, "+-"[p % 2]))
    universe = sorted(set(universe), key=lambda r: (r[0], r[1]))
    texts = []
    for s in range(3):
        rows = thin(rng, universe, 9 + 4 * s)
        if s == 1:
            rows = rows + [(3, 100 + 7 * i, "+") for i in range(25)]                # a chromosome the others lack
        lines = [M.site_line(c, p, st, "UIM"[int(rng.integers(3))], [0.9999, 0.7][int(rng.integers(8) == 0)],
                             round(float(rng.random()), 4)) for c, p, st in rows]
        texts.append(mark(Deferring(G.text(lines))))
    args = M.Args(cutoff=2048, step=5, size=5, absolute=False, flt=FLT)
    kw = dict(cutoff=args.cutoff, cutoff_gene_length=False, step=5, size=5, absolute=False, counts=M.windows_new(args, 100))
    genes = abn.Genes(gpu_ctx, G.gene_lists(genome))
    sites = []
    for d in texts:
        r = gpu_ctx.parse_sites_resident(d.text(), slab_bytes=d.slab)
        r.insert(*decide(L, d.text(), r.deferred()))
        assert r.info()["n_deferred"] >= len(d.marked) >= 4 and len(slabs(d.text(), d.slab)) >= 3
        sites.append(r)
    fetched = [r.fetch() for r in sites]
    masks, n_common = common_masks(fetched)
    assert len({len(f["line"]) for f in fetched}) == 3 and 1000 < n_common < min(len(f["line"]) for f in fetched)
    off = np.arange(4, dtype=np.int64) * n_common
    cat = lambda k: np.concatenate([f[k][m] for f, m in zip(fetched, masks)])
    with np.errstate(invalid="ignore"):
        code = (cat("status") | np.where(cat("posteriormax") < FLT, 0x80, 0)).astype(np.uint8)
    before = abn.Windows.from_parsed(gpu_ctx, genes, sites, posterior_max_filter=FLT, **kw)
    want = abn.Windows.from_sites(gpu_ctx, genes, off, cat("chromosome"), cat("start"), cat("end"), cat("strand"), code,
                                  cat("meth_lvl"), **kw)
    got = abn.Windows.from_parsed(gpu_ctx, genes, sites, posterior_max_filter=FLT, align=True, **kw)
    after = abn.Windows.from_parsed(gpu_ctx, genes, sites, posterior_max_filter=FLT, **kw)
    try:
        assert before.layout()[2].any()                                             # unaligned: a ragged window, which fails
        assert not got.layout()[2].any() and got.stats()[0].sum() > 1000
        assert (got.W, got.row_stride, got.n_sites, got.n_samples) == (want.W, want.row_stride, want.n_sites, want.n_samples)
        for x, y in zip(want.stats() + want.layout(), got.stats() + got.layout()):   # counts, sums bit for bit, kept; layout
            assert x.dtype == y.dtype and x.tobytes() == y.tobytes()
        assert np.array_equal(want.packed(), got.packed())
        for x, y in zip(want.pairwise(), got.pairwise()):
            assert x.tobytes() == y.tobytes()
        b, n, ms = got.common()
        assert b.tolist() == [len(f["line"]) for f in fetched] and n == n_common and ms.shape == (4,) and np.all(ms > 0)
        b, n, ms = before.common()                                                  # a handle made any other way
        assert b.tolist() == [len(f["line"]) for f in fetched] and n == -1 and not ms.any()
        assert want.common()[0].tolist() == [n_common] * 3
        for x, y in zip(before.stats() + before.layout() + (before.packed(),), after.stats() + after.layout() + (after.packed(),)):
            assert x.tobytes() == y.tobytes()                                       # the resident handles are unchanged
        for f, r in zip(fetched, sites):
            P.assert_sites_equal(r.fetch(), f, list(f))
    finally:
        for h in [before, want, got, after, genes] + sites:
            h.close()


def codes_methylome(rng, universe, lose, extra=()):
    """a methylome text over the CG positions of `universe` without `lose` of them, rows of other contexts (no site)
    between, posteriors on both sides of the filter and at it, levels of -0.0 among the others"""
    rows = []
    for chrom, pos, strand in thin(rng, universe, lose) + list(extra):
        if rng.integers(4) == 0:
            rows.append(P.cg_line(chrom=str(chrom), pos=str(pos), ctx=("CHH", "CHG")[int(rng.integers(2))], tri="CCT"))
        post = ("0.9999", "0.99", f"{rng.random():.4f}", "0.5")[int(rng.integers(4))]
        level = "-0.0" if rng.integers(5) == 0 else f"{rng.random():.4f}"
        rows.append(P.cg_line(chrom=str(chrom), pos=str(pos), strand=strand, pm=post, st="UIM"[int(rng.integers(3))], ml=level,
                              tri="CGA"))
    return P.HEADER + "".join(r + "\n" for r in rows)


@pytest.mark.parametrize("slab_bytes", [0, 4096, 300])
def test_codes_aligned_equals_the_model_on_the_filtered_sequences(abn, gpu_ctx, L, slab_bytes):
    rng = np.random.default_rng(300 + slab_bytes)
    universe = [(c, p, "+-"[p % 2]) for c in (1, 10, 2) for p in sorted(set(rng.integers(1, 4000, size=400).tolist()))]
    samples = [Deferring(codes_methylome(rng, universe, 5 + 3 * s, [("M", 9 + i, "+") for i in range(4)] if s == 2 else ()))
               for s in range(4)]
    for d in samples:
        d.slab = slab_bytes or 1 << 26
        mark(d)
    texts = [d.text() for d in samples]
    merged = [P.device_sites_merged(L, t, 0, slab_bytes)[0] for t in texts]
    masks, n_common = common_masks(merged)
    counts = [len(m["line"]) for m in merged]
    assert len(set(counts)) > 1 and 1025 < n_common < min(counts)
    inserted = sum(len(d.marked & set(m["line"].tolist())) for d, m in zip(samples, merged))
    assert inserted >= 4
    want_packed = K.packed_rows(abn, [K.code_bytes(m["status"][k], m["posteriormax"][k]) for m, k in zip(merged, masks)])
    folds = [K.fold(m["posteriormax"][k], m["meth_lvl"][k]) for m, k in zip(merged, masks)]
    sites = []
    for t in texts:
        r = gpu_ctx.parse_sites_resident(t, skip_lines=0, slab_bytes=slab_bytes)
        r.insert(*decide(L, t, r.deferred()))
        sites.append(r)
    plain = abn.Codes.from_parsed(gpu_ctx, sites, posterior_max_filter=FLT)
    got = abn.Codes.from_parsed(gpu_ctx, sites, posterior_max_filter=FLT, align=True)
    again = abn.Codes.from_parsed(gpu_ctx, sites, posterior_max_filter=FLT)
    try:
        with pytest.raises(abn.AbnError) as e:                                      # unaligned: still refused
            plain.pairwise()
        assert e.value.status == INVALID and "differ in length" in str(e.value)
        assert got.info() == {"n_samples": 4, "n_sites": n_common, "row_stride": max(abn.packed_row_stride(n_common), 64),
                              "same_len": True}
        assert got.packed().tobytes() == want_packed.tobytes()                      # padding included
        count, lsk, kept = got.stats()
        assert count.tolist() == [n_common] * 4 and kept.tolist() == [k for _, k in folds]
        assert [struct.pack("<d", v) for v in lsk] == [s for s, _ in folds]          # the folds bit for bit
        for x, y in zip(got.pairwise(), gpu_ctx.pairwise_divergence_packed(want_packed, n_common)):
            assert x.dtype == y.dtype and x.tobytes() == y.tobytes()
        b, n, ms = got.common()
        assert b.tolist() == counts and n == n_common and np.all(ms > 0)
        b, n, ms = plain.common()
        assert b.tolist() == counts and n == -1 and not ms.any()
        assert plain.packed().tobytes() == again.packed().tobytes()                 # the resident handles are unchanged
        assert all(x.tobytes() == y.tobytes() for x, y in zip(plain.stats(), again.stats()))
        assert plain.stats()[0].tolist() == counts
    finally:
        for h in [plain, got, again] + sites:
            h.close()


def test_aligned_refusals_and_small_cases(abn, gpu_ctx, L):
    """samples whose runs come in different orders give no handle; no common site, one sample and empty samples do"""
    row = lambda c, p: P.cg_line(chrom=str(c), pos=str(p), tri="CGA")
    text = lambda rows: (P.HEADER + "".join(r + "\n" for r in rows)).encode()
    a = text([row(1, p) for p in range(5, 45)] + [row(2, p) for p in range(5, 45)])
    b = text([row(2, p) for p in range(5, 45)] + [row(1, p) for p in range(5, 46)])
    split = text([row(1, 5), row(2, 5), row(1, 6)])
    genes = abn.Genes(gpu_ctx, [(1, 0, [1], [100], [0])])
    kw = dict(cutoff=100, step=5, size=5, absolute=False, counts=M.windows_new(M.Args(cutoff=100), 100))
    parse = lambda t: gpu_ctx.parse_sites_resident(t, skip_lines=0)
    for texts, words in (([a, b], "sample 1, site 0: not co-ordered"), ([a, split], "sample 1, site 2: split run")):
        sites = [parse(t) for t in texts]
        for make in (lambda: abn.Codes.from_parsed(gpu_ctx, sites, posterior_max_filter=FLT, align=True),
                     lambda: abn.Windows.from_parsed(gpu_ctx, genes, sites, posterior_max_filter=FLT, align=True, **kw)):
            with pytest.raises(abn.AbnError) as e:
                make()
            assert e.value.status == INVALID and words in str(e.value), str(e.value)
        for s in sites:
            s.close()
    other = text([row(3, p) for p in range(5, 45)])
    for texts, n_common in (([a, other], 0), ([a], 80), ([a, b""], 0), ([b""], 0), ([a, a, a], 80)):
        sites = [parse(t) for t in texts]
        c = abn.Codes.from_parsed(gpu_ctx, sites, posterior_max_filter=FLT, align=True)
        w = abn.Windows.from_parsed(gpu_ctx, genes, sites, posterior_max_filter=FLT, align=True, **kw)
        assert c.common()[1] == w.common()[1] == n_common and c.info()["n_sites"] == n_common and c.info()["same_len"]
        assert c.stats()[0].tolist() == [n_common] * len(texts)
        if n_common == 0:
            assert set(c.packed().ravel().tolist()) == {0xff} and not w.stats()[0].any()
        if len(texts) == 3:
            full = abn.Codes.from_parsed(gpu_ctx, sites, posterior_max_filter=FLT)      # every site common: the unaligned handle
            assert full.packed().tobytes() == c.packed().tobytes()
            assert all(x.tobytes() == y.tobytes() for x, y in zip(full.stats(), c.stats()))
            full.close()
        for h in [c, w] + sites:
            h.close()
    genes.close()


# ---------------------------------------------------------------- the tools
NAMES = ("G0.txt", "G4_2.txt", "G4_8.txt")


def tool_inputs(tmp_path):
    """three small methylomes of a few hundred CG rows around the first genes of the bundled annotation, each lacking a few
    rows the others have, the second with a chromosome of its own; the same files without the rows outside the common set;
    a nodelist for either directory and the edgelist.  -> (edgelist, {"raw" | "filtered": (directory, nodelist)})"""
    genome, genes = M.genome_of((GOLDEN / "annotation.txt").read_text())
    rng = np.random.default_rng(8)
    where = set()
    for g in sorted(genes, key=lambda g: (g["chromosome"], g["start"]))[:3]:
        where |= {(g["chromosome"], int(p), "+-*"[g["strand"]].replace("*", "+"))
                  for p in rng.integers(g["start"] - 2100, g["end"] + 2100, size=130)}
    where = sorted(where)
    status = rng.choice([0, 2], size=len(where), p=[0.6, 0.4])
    rows = []
    for k in range(3):
        flip = rng.random(len(where)) < 0.05 * (k + 1)
        status = np.where(flip, rng.integers(0, 3, size=len(where)), status)
        mine = [(key, M.site_line(*key, "UIM"[int(s)], [0.9999, 0.7][int(rng.integers(10) == 0)],
                                  round(float(0.05 + 0.45 * s + 0.04 * rng.random()), 4))) for key, s in zip(where, status)]
        mine = thin(rng, mine, 4 + 2 * k)
        if k == 1:
            mine += [((2, 50 + 9 * i, "+"), M.site_line(2, 50 + 9 * i, "+", "M", 0.9999, 0.5)) for i in range(12)]
        rows.append(mine)
    common = set.intersection(*({key for key, _ in mine} for mine in rows))
    assert 300 < len(common) < min(len(m) for m in rows) and len({len(m) for m in rows}) == 3
    out = {}
    for side in ("raw", "filtered"):
        meth = tmp_path / side
        meth.mkdir()
        for name, mine in zip(NAMES, rows):
            (meth / name).write_text(M.HEADER + "".join(line + "\n" for key, line in mine if side == "raw" or key in common))
        nodes = "filename\tnode\tgen\tmeth\n" + "".join(
            f"{f}\t{node}\t{gen}\t{m}\n" for f, node, gen, m in
            [(f"{meth}/G0.txt", "0_0", 0, "Y"), ("-", "1_2", 1, "N"), ("-", "1_8", 1, "N"), ("-", "2_2", 2, "N"), ("-", "2_8", 2, "N"),
             ("-", "3_2", 3, "N"), ("-", "3_8", 3, "N"), (f"{meth}/G4_2.txt", "4_2", 4, "Y"), (f"{meth}/G4_8.txt", "4_8", 4, "Y")])
        (tmp_path / f"nodelist_{side}.fn").write_text(nodes)
        out[side] = (meth, tmp_path / f"nodelist_{side}.fn")
    (tmp_path / "edgelist.fn").write_text((GOLDEN / "data" / "edgelist.txt").read_text())
    return tmp_path / "edgelist.fn", out


def run_tool(cmd, out, hide):
    """-> (the output directory's files, stdout without the per-sample lines of --align and without the paths in `hide`)"""
    out.mkdir()
    r = subprocess.run([*map(str, cmd), "-o", str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    text = r.stdout
    for h in hide + [out]:
        text = text.replace(str(h), "DIR")
    aligned = [l for l in text.splitlines() if l.startswith("Aligned by position: ")]
    rest = "".join(l + "\n" for l in text.splitlines() if not l.startswith("Aligned by position: "))
    return {p.name: p.read_bytes() for p in sorted(out.iterdir()) if p.is_file()}, rest, aligned, r.stderr


def test_alphabeta_align_position_equals_the_filtered_files(tmp_path):
    from alphabeta_rs_amd import build as B

    B.build_host()
    edges, sides = tool_inputs(tmp_path)
    base = lambda side: [B.CLI, "-i", "20", "-n", sides[side][1], "-e", edges, "--parse", "device", "--sites", "device"]
    hide = [sides["raw"][0], sides["filtered"][0], sides["raw"][1], sides["filtered"][1]]
    got = run_tool(base("raw") + ["--align", "position"], tmp_path / "out_aligned", hide)
    want = run_tool(base("filtered") + ["--align", "none"], tmp_path / "out_filtered", hide)
    assert set(want[0]) >= {"pedigree.txt", "analysis.txt", "raw.npy"} and sorted(got[0]) == sorted(want[0])
    for name in want[0]:
        assert got[0][name] == want[0][name], name
    assert got[1] == want[1] and got[3] == want[3] and "Lengths do not match" not in got[1]
    assert len(got[2]) == 3 and not want[2]
    for line, name in zip(got[2], NAMES):                                           # its name, its sites, the number kept
        assert name in line and line.split(": ")[-1].split(" sites, ")[1].endswith(" kept"), line
    kept = {l.split(" sites, ")[1] for l in got[2]}
    assert len(kept) == 1 and len({l.split(": ")[-1].split(" sites, ")[0] for l in got[2]}) == 3
    none = run_tool(base("raw") + ["--align", "none"], tmp_path / "out_none", hide)
    assert "Lengths do not match" in none[1] and none[0]["pedigree.txt"] != got[0]["pedigree.txt"]
    r = subprocess.run([str(B.CLI), "-n", str(sides["raw"][1]), "-e", str(edges), "-o", str(tmp_path), "--align", "position"],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--align position needs --sites device" in r.stderr
    r = subprocess.run([str(B.CLI), "--align", "sites"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--align expects none or position" in r.stderr


def test_metaprofile_align_position_equals_the_filtered_files(tmp_path):
    from alphabeta_rs_amd import build as B

    B.build_host()
    edges, sides = tool_inputs(tmp_path)
    base = lambda side: [B.META_CLI, "--methylome", sides[side][0], "--genome", GOLDEN / "annotation.txt", "--nodes",
                         sides[side][1], "--edges", edges, "--iterations", "5", "--seed", "77", "-s", "5", "-w", "5", "-c",
                         "2048", "--sites", "device"]
    hide = [sides["raw"][0], sides["filtered"][0], sides["raw"][1], sides["filtered"][1]]
    got = run_tool(base("raw") + ["--align", "position"], tmp_path / "out_aligned", hide)
    want = run_tool(base("filtered") + ["--align", "none"], tmp_path / "out_filtered", hide)
    assert sorted(got[0]) == sorted(want[0]) and len(want[0]) >= 8 and {"results.txt", "raw.npy", "distributions.txt"} <= set(want[0])
    for name in want[0]:
        assert got[0][name] == want[0][name], name
    assert len(want[0]["results.txt"].splitlines()) > 10
    assert got[1] == want[1] and got[3] == want[3] and len(got[2]) == 3 and not want[2]
    assert "site counts differ" not in got[1]
    none = run_tool(base("raw"), tmp_path / "out_none", hide)                        # unaligned: ragged windows fail
    assert "site counts differ" in none[1] and "Lengths do not match" in none[1]
    r = subprocess.run([str(B.META_CLI), "-o", str(tmp_path), *map(str, base("raw")[1:-2]), "--align", "position"],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--align position needs --sites device" in r.stderr
    r = subprocess.run([str(B.META_CLI), "-o", str(tmp_path), "--align", "sites"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--align expects none or position" in r.stderr
