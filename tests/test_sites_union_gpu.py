"""Methylomes aligned on the union of their sites on the device (abn_sites_union, abn_windows_create_union,
abn_codes_create_union; alphabeta_rs_amd/csrc/abn_sites_union.hpp).  The oracle is what the project already has, fed padded
input: the union is computed here from sets of key tuples and a sort (tests/_union_model.py), a row of status U, posterior 0
and level 0 is inserted in Python wherever a sample lacks a key, and the union result must be byte-identical to the existing
unaligned path on the padded input."""
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

import _codes_model as K
import _common_model as X
import _genes_model as G
import _parse_model as P
import _union_model as U
import _windows_model as M
from test_sites_common_gpu import codes_methylome, keys_of, mark, thin
from test_sites_resident_gpu import Deferring, decide, slabs

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden"
FLT = K.FILTER
INVALID = 1  # ABN_ERR_INVALID_ARG


@pytest.fixture(scope="module")
def L():
    return P.hostlib()


# ---------------------------------------------------------------- the step alone
def device(ctx, samples):
    """Context.union_sites -> ("ok", dest per sample, n_union)"""
    off, chrom, start, end, strand = X.concat(samples)
    dest, n = ctx.union_sites(off, chrom, start, end, strand)
    assert dest.dtype == np.uint32 and dest.shape == (int(off[-1]),)
    return ("ok", [dest[off[s]:off[s + 1]] for s in range(len(samples))], n)


def assert_same(got, want, name):
    assert want[0] == "ok" and got[2] == want[2], (name, got[2], want[:3:2])
    for g, w in zip(got[1], want[1]):
        assert g.tobytes() == w.tobytes(), name


def test_union_sites_against_the_sorted_set(gpu_ctx):
    seen = np.zeros(5, dtype=np.int64)
    for name, samples, total in U.generated_cases():
        want = U.model(samples)
        assert_same(device(gpu_ctx, samples), want, name)
        seen += U.coverage(samples, want[3])
    assert seen.min() >= 5, seen.tolist()


def test_union_sites_edges(gpu_ctx):
    key = lambda i, c=1: (c, 10 + i, 11 + i, i % 3)
    big = [key(i) for i in range(3000)]
    edge = [key(i, 1) for i in range(256)] + [key(i, 2) for i in range(300)]          # a run boundary on site 256
    other = [key(i, 1) for i in range(0, 400, 2)] + [key(i, 2) for i in range(1, 500)]
    for name, samples, n_union in (
            ("one sample", [big[:300]], 300),
            ("one empty sample", [[]], 0),
            ("empty samples alone", [[], [], []], 0),
            ("an empty sample among others", [big[:10], [], big[5:15]], 15),
            ("an empty first sample", [[], big[:10]], 10),
            ("disjoint", [big[:100], big[100:200]], 200),
            ("disjoint, interleaved", [big[0:200:2], big[1:200:2]], 200),
            ("identical", [big[:257], big[:257], big[:257]], 257),
            ("1 and 3000", [[big[1234]], big], 3000),
            ("3000 and 1 below all", [big, [(1, 5, 5, 0)]], 3001),
            ("only end differs", [[(1, 5, 6, 0), (1, 5, 7, 0)], [(1, 5, 7, 0)]], 2),
            ("only strand differs", [[(1, 5, 6, 0), (1, 5, 6, 2)], [(1, 5, 6, 1), (1, 5, 6, 2)]], 3),
            ("only the chromosome differs", [[(1, 5, 6, 0)], [(2, 5, 6, 0)]], 2),
            ("a chromosome only the last sample has", [big[:50], big[:50], big[:40] + [key(i, 2) for i in range(9)]], 59),
            ("a run boundary on site 256", [edge, other + [key(0, 3)]], 328 + 500 + 1),
            ("a run boundary on site 256, the second sample's", [other[:100], edge], len(set(other[:100]) | set(edge))),
            ("runs 1, 10, 2 with organelles", [[key(0, 1), key(0, 10), key(0, 2), key(0, 256), key(0, 257)],
                                                [key(0, 1), key(1, 10), key(0, 2), key(0, 257)]], 6)):
        want = U.model(samples)
        assert want[2] == n_union, name
        assert_same(device(gpu_ctx, samples), want, name)
    got = device(gpu_ctx, [big[:257]] * 3)                                           # identical: dest is the identity
    assert all(d.tolist() == list(range(257)) for d in got[1]) and got[2] == 257


def test_union_sites_refusals(abn, gpu_ctx):
    rng = np.random.default_rng(7)
    cases = [(name, samples, kind) for name, samples, kind in X.refusal_cases(rng) if kind in (X.SPLIT, X.NOT_ASCENDING)]
    cases += [(name, samples, U.RUN_ORDER) for name, samples, _, _ in U.run_order_cases()]
    kinds = {U.SPLIT: 0, U.NOT_ASCENDING: 0, U.RUN_ORDER: 0}
    for name, samples, kind in cases:
        want = U.model(samples)
        assert want[:2] == ("refused", kind), (name, want)
        with pytest.raises(abn.AbnError) as e:
            device(gpu_ctx, samples)
        assert e.value.status == INVALID, name
        assert f"sample {want[2]}, site {want[3]}: {U.WORDS[kind]}" in str(e.value), (name, str(e.value), want)
        kinds[kind] += 1
    assert min(kinds.values()) >= 3, kinds
    with pytest.raises(abn.AbnError) as e:                                          # no index into the table of runs
        device(gpu_ctx, [[(1, 1, 1, 0)], [(1, 1, 1, 0), (258, 1, 1, 0)]])
    assert e.value.status == INVALID and "sample 1, site 1" in str(e.value)
    lib = gpu_ctx._L                                                               # the argument checks of the siblings
    off = np.array([0, 0], dtype=np.int64)
    n = np.zeros(1, dtype=np.int64)
    i64 = lambda a: a.ctypes.data_as(lib.abn_sites_union.argtypes[2])
    assert lib.abn_sites_union(None, 1, i64(off), None, None, None, None, None, i64(n)) == INVALID
    assert lib.abn_sites_union(gpu_ctx._h, 0, i64(off), None, None, None, None, None, i64(n)) == INVALID
    assert lib.abn_sites_union(gpu_ctx._h, 1, None, None, None, None, None, None, i64(n)) == INVALID
    assert lib.abn_sites_union(gpu_ctx._h, 1, i64(off), None, None, None, None, None, None) == INVALID
    assert lib.abn_sites_union(gpu_ctx._h, 1, i64(np.array([0, 3], dtype=np.int64)), None, None, None, None, None, i64(n)) == INVALID
    assert lib.abn_sites_union(gpu_ctx._h, 1, i64(off), None, None, None, None, None, i64(n)) == 0 and n[0] == 0


# ---------------------------------------------------------------- samples that share most of their sites
def pad(records, fill):
    """records: per sample a dict of arrays with chromosome, start, end, strand and the columns of `fill` ({column: the
    placeholder's value}) -> (the same columns over the union, n_union per sample; the model's result)"""
    keys = [keys_of(r) for r in records]
    want = U.model(keys)
    assert want[0] == "ok", want
    cols = list(zip(*want[3])) if want[3] else [(), (), (), ()]
    out = []
    for r, dest in zip(records, want[1]):
        row = {k: np.array(c, dtype=r[k].dtype) for k, c in zip(("chromosome", "start", "end", "strand"), cols)}
        for k, v in fill.items():
            row[k] = np.full(want[2], v, dtype=r[k].dtype)
            row[k][dest] = r[k]
        out.append(row)
    return out, want


FILL = {"status": 0, "posteriormax": 0.0, "meth_lvl": 0.0}                          # status U, filtered, level +0.0


def test_windows_union_equals_from_sites_on_the_padded_arrays(abn, gpu_ctx, L):
    rng = np.random.default_rng(12)
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
    rows, model = pad(fetched, FILL)
    n_union = model[2]
    counts = [len(f["line"]) for f in fetched]
    assert len(set(counts)) == 3 and n_union > max(counts) > 1000
    off = np.arange(4, dtype=np.int64) * n_union
    cat = lambda k: np.concatenate([r[k] for r in rows])
    code = K.code_bytes(cat("status"), cat("posteriormax"))
    before = abn.Windows.from_parsed(gpu_ctx, genes, sites, posterior_max_filter=FLT, **kw)
    want = abn.Windows.from_sites(gpu_ctx, genes, off, cat("chromosome"), cat("start"), cat("end"), cat("strand"), code,
                                  cat("meth_lvl"), **kw)
    got = abn.Windows.from_parsed(gpu_ctx, genes, sites, posterior_max_filter=FLT, align="union", **kw)
    after = abn.Windows.from_parsed(gpu_ctx, genes, sites, posterior_max_filter=FLT, **kw)
    try:
        assert before.layout()[2].any()                                             # unaligned: a ragged window, which fails
        assert not got.layout()[2].any() and got.stats()[0].sum() > 1000            # no ragged window
        assert (got.W, got.row_stride, got.n_sites, got.n_samples) == (want.W, want.row_stride, want.n_sites, want.n_samples)
        for x, y in zip(want.stats() + want.layout(), got.stats() + got.layout()):   # counts, sums bit for bit, kept; layout
            assert x.dtype == y.dtype and x.tobytes() == y.tobytes()
        assert np.array_equal(want.packed(), got.packed())
        for x, y in zip(want.pairwise(), got.pairwise()):
            assert x.tobytes() == y.tobytes()
        b, n, ms = got.union()
        assert b.tolist() == counts and n == n_union and ms.shape == (8,) and np.all(ms > 0)
        assert got.common()[1] == -1
        b, n, ms = before.union()                                                   # a handle made any other way
        assert b.tolist() == counts and n == -1 and not ms.any()
        for x, y in zip(before.stats() + before.layout() + (before.packed(),), after.stats() + after.layout() + (after.packed(),)):
            assert x.tobytes() == y.tobytes()                                       # the resident handles are unchanged
        for f, r in zip(fetched, sites):
            P.assert_sites_equal(r.fetch(), f, list(f))
    finally:
        for h in [before, want, got, after, genes] + sites:
            h.close()


def assert_codes_equal_the_model(abn, ctx, got, merged, plain=None):
    """a union Codes handle against _codes_model on the padded sequences of `merged` (per sample, the merged records)"""
    rows, model = pad(merged, FILL)
    n, n_union = len(merged), model[2]
    want_packed = K.packed_rows(abn, [K.code_bytes(r["status"], r["posteriormax"]) for r in rows])
    folds = [K.fold(r["posteriormax"], r["meth_lvl"]) for r in rows]
    assert got.info() == {"n_samples": n, "n_sites": n_union, "row_stride": max(abn.packed_row_stride(n_union), 64),
                          "same_len": True}
    assert got.packed().tobytes() == want_packed.tobytes()                          # padding included
    count, lsk, kept = got.stats()
    assert count.tolist() == [n_union] * n and kept.tolist() == [k for _, k in folds]
    assert [struct.pack("<d", v) for v in lsk] == [s for s, _ in folds]              # the folds bit for bit
    if plain is not None:                                                           # ... and the unaligned handle's
        _, plain_lsk, plain_kept = plain.stats()
        assert kept.tobytes() == plain_kept.tobytes() and lsk.tobytes() == plain_lsk.tobytes()
    if n >= 2 and n_union > 0:
        for x, y in zip(got.pairwise(), ctx.pairwise_divergence_packed(want_packed, n_union)):
            assert x.dtype == y.dtype and x.tobytes() == y.tobytes()
    b, nu, ms = got.union()
    assert b.tolist() == [len(m["line"]) for m in merged] and nu == n_union and ms.shape == (8,)
    assert got.common()[1] == -1
    return n_union


@pytest.mark.parametrize("slab_bytes", [0, 4096, 300])
def test_codes_union_equals_the_model_on_the_padded_sequences(abn, gpu_ctx, L, slab_bytes):
    rng = np.random.default_rng(400 + slab_bytes)
    universe = [(c, p, "+-"[p % 2]) for c in (1, 10, 2) for p in sorted(set(rng.integers(1, 4000, size=400).tolist()))]
    samples = [Deferring(codes_methylome(rng, universe, 5 + 3 * s, [("M", 9 + i, "+") for i in range(4)] if s == 2 else ()))
               for s in range(4)]
    for d in samples:
        d.slab = slab_bytes or 1 << 26
        mark(d)
    texts = [d.text() for d in samples]
    merged = [P.device_sites_merged(L, t, 0, slab_bytes)[0] for t in texts]
    counts = [len(m["line"]) for m in merged]
    inserted = sum(len(d.marked & set(m["line"].tolist())) for d, m in zip(samples, merged))
    assert len(set(counts)) > 1 and inserted >= 4
    sites = []
    for t in texts:
        r = gpu_ctx.parse_sites_resident(t, skip_lines=0, slab_bytes=slab_bytes)
        r.insert(*decide(L, t, r.deferred()))
        sites.append(r)
    plain = abn.Codes.from_parsed(gpu_ctx, sites, posterior_max_filter=FLT)
    got = abn.Codes.from_parsed(gpu_ctx, sites, posterior_max_filter=FLT, align="union")
    again = abn.Codes.from_parsed(gpu_ctx, sites, posterior_max_filter=FLT)
    try:
        n_union = assert_codes_equal_the_model(abn, gpu_ctx, got, merged, plain)
        assert n_union > max(counts) > 1025 and np.all(got.union()[2] > 0)
        b, n, ms = plain.union()
        assert b.tolist() == counts and n == -1 and not ms.any()
        assert plain.packed().tobytes() == again.packed().tobytes()                 # the resident handles are unchanged
        assert all(x.tobytes() == y.tobytes() for x, y in zip(plain.stats(), again.stats()))
        assert plain.stats()[0].tolist() == counts
    finally:
        for h in [plain, got, again] + sites:
            h.close()


def test_union_refusals_and_small_cases(abn, gpu_ctx, L):
    """samples whose runs come in different orders give no handle; no site, one sample, an empty sample among others,
    identical samples and disjoint samples do, through both handles"""
    row = lambda c, p: P.cg_line(chrom=str(c), pos=str(p), tri="CGA")
    text = lambda rows: (P.HEADER + "".join(r + "\n" for r in rows)).encode()
    a = text([row(1, p) for p in range(5, 45)] + [row(2, p) for p in range(5, 45)])
    b = text([row(2, p) for p in range(5, 45)] + [row(1, p) for p in range(5, 46)])
    split = text([row(1, 5), row(2, 5), row(1, 6)])
    genes = abn.Genes(gpu_ctx, [(1, 0, [1], [100], [0])])
    kw = dict(cutoff=100, step=5, size=5, absolute=False, counts=M.windows_new(M.Args(cutoff=100), 100))
    parse = lambda t: gpu_ctx.parse_sites_resident(t, skip_lines=0)
    for texts, words in (([a, b], "sample 1, site 40: run order"), ([a, split], "sample 1, site 2: split run")):
        sites = [parse(t) for t in texts]
        for make in (lambda: abn.Codes.from_parsed(gpu_ctx, sites, posterior_max_filter=FLT, align="union"),
                     lambda: abn.Windows.from_parsed(gpu_ctx, genes, sites, posterior_max_filter=FLT, align="union", **kw)):
            with pytest.raises(abn.AbnError) as e:
                make()
            assert e.value.status == INVALID and words in str(e.value), str(e.value)
        for s in sites:
            s.close()
    with pytest.raises(ValueError):
        abn.Codes.from_parsed(gpu_ctx, [], posterior_max_filter=FLT, align="sites")
    other = text([row(3, p) for p in range(5, 45)])
    for texts, n_union in (([b""], 0), ([b"", b""], 0), ([a], 80), ([a, b""], 80), ([b"", a, b""], 80), ([a, a, a], 80),
                           ([a, other], 120)):
        sites = [parse(t) for t in texts]
        merged = [P.device_sites_merged(L, t, 0, 0)[0] for t in texts]
        c = abn.Codes.from_parsed(gpu_ctx, sites, posterior_max_filter=FLT, align="union")
        w = abn.Windows.from_parsed(gpu_ctx, genes, sites, posterior_max_filter=FLT, align="union", **kw)
        full = abn.Codes.from_parsed(gpu_ctx, sites, posterior_max_filter=FLT)
        assert assert_codes_equal_the_model(abn, gpu_ctx, c, merged, full) == n_union == w.union()[1]
        assert not w.layout()[2].any()
        if n_union == 0:
            assert set(c.packed().ravel().tolist()) == {0xff} and not w.stats()[0].any()
        else:
            assert len({tuple(r) for r in w.stats()[0].tolist()}) == 1              # every sample has every window's sites
        if len(texts) == 3 and texts[0] == texts[1] == texts[2]:                                  # identical: the unaligned handle
            assert full.packed().tobytes() == c.packed().tobytes()
            assert all(x.tobytes() == y.tobytes() for x, y in zip(full.stats(), c.stats()))
        if b"" in texts and n_union:                                                # the empty sample: a row of placeholders
            s = texts.index(b"")
            assert set(c.packed()[s, :n_union // 4].tolist()) == {0xff} and c.stats()[2][s] == 0
        if len(texts) == 2 and n_union:                                             # [a, empty] and [a, other]: no site compared
            assert c.pairwise()[1].tolist() == [0]
        for h in [c, w, full] + sites:
            h.close()
    genes.close()


# ---------------------------------------------------------------- the tools
NAMES = ("G0.txt", "G4_2.txt", "G4_8.txt")


def tool_inputs(tmp_path):
    """three small methylomes of a few hundred CG rows around the first genes of the bundled annotation, each lacking a few
    rows the others have, the second with a chromosome of its own; the same files with a row of status U, posterior 0.0 and
    level 0.0 wherever a file lacks a row another has; a nodelist for either directory and the edgelist.
    -> (edgelist, {"raw" | "padded": (directory, nodelist)}, sites per raw file, n_union)"""
    genome, genes = M.genome_of((GOLDEN / "annotation.txt").read_text())
    rng = np.random.default_rng(9)
    where = {}
    first = sorted(genes, key=lambda g: (g["chromosome"], g["start"]))[:3]
    assert {g["chromosome"] for g in first} == {1}
    for g in first:
        for p in rng.integers(g["start"] - 2100, g["end"] + 2100, size=130):
            where.setdefault((1, int(p)), "+-*"[g["strand"]].replace("*", "+"))          # one row per position
    where = [(c, p, st) for (c, p), st in sorted(where.items())]
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
    union = sorted(set().union(*({key for key, _ in mine} for mine in rows)))          # chromosome 1, then 2: the run order
    assert len(union) > max(len(m) for m in rows) and len({len(m) for m in rows}) == 3
    out = {}
    for side in ("raw", "padded"):
        meth = tmp_path / side
        meth.mkdir()
        for name, mine in zip(NAMES, rows):
            have = dict(mine)
            lines = [line for _, line in mine] if side == "raw" else [have.get(key) or M.site_line(*key, "U", 0.0, 0.0)
                                                                      for key in union]
            (meth / name).write_text(M.HEADER + "".join(line + "\n" for line in lines))
        nodes = "filename\tnode\tgen\tmeth\n" + "".join(
            f"{f}\t{node}\t{gen}\t{m}\n" for f, node, gen, m in
            [(f"{meth}/G0.txt", "0_0", 0, "Y"), ("-", "1_2", 1, "N"), ("-", "1_8", 1, "N"), ("-", "2_2", 2, "N"), ("-", "2_8", 2, "N"),
             ("-", "3_2", 3, "N"), ("-", "3_8", 3, "N"), (f"{meth}/G4_2.txt", "4_2", 4, "Y"), (f"{meth}/G4_8.txt", "4_8", 4, "Y")])
        (tmp_path / f"nodelist_{side}.fn").write_text(nodes)
        out[side] = (meth, tmp_path / f"nodelist_{side}.fn")
    (tmp_path / "edgelist.fn").write_text((GOLDEN / "data" / "edgelist.txt").read_text())
    return tmp_path / "edgelist.fn", out, [len(m) for m in rows], len(union)


def run_tool(cmd, out, hide):
    """-> (the output directory's files, stdout without the per-sample lines of --align union and without the paths in
    `hide`, those lines, stderr)"""
    out.mkdir()
    r = subprocess.run([*map(str, cmd), "-o", str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    text = r.stdout
    for h in hide + [out]:
        text = text.replace(str(h), "DIR")
    aligned = [l for l in text.splitlines() if l.startswith("Aligned by union: ")]
    rest = "".join(l + "\n" for l in text.splitlines() if not l.startswith("Aligned by union: "))
    return {p.name: p.read_bytes() for p in sorted(out.iterdir()) if p.is_file()}, rest, aligned, r.stderr


def assert_union_lines(lines, counts, n_union):
    assert len(lines) == 3
    for line, name, count in zip(lines, NAMES, counts):                             # its name, its sites, the union's
        assert name in line and line.endswith(f": {count} sites, {n_union} in the union"), line


def test_alphabeta_align_union_equals_the_padded_files(tmp_path):
    from alphabeta_rs_amd import build as B

    B.build_host()
    edges, sides, counts, n_union = tool_inputs(tmp_path)
    base = lambda side: [B.CLI, "-i", "20", "-n", sides[side][1], "-e", edges, "--parse", "device", "--sites", "device"]
    hide = [sides["raw"][0], sides["padded"][0], sides["raw"][1], sides["padded"][1]]
    got = run_tool(base("raw") + ["--align", "union"], tmp_path / "out_union", hide)
    want = run_tool(base("padded") + ["--align", "none"], tmp_path / "out_padded", hide)
    assert set(want[0]) >= {"pedigree.txt", "analysis.txt", "raw.npy"} and sorted(got[0]) == sorted(want[0])
    for name in want[0]:
        assert got[0][name] == want[0][name], name
    assert got[1] == want[1] and got[3] == want[3] and "Lengths do not match" not in got[1]
    assert not want[2]
    assert_union_lines(got[2], counts, n_union)
    r = subprocess.run([str(B.CLI), "-n", str(sides["raw"][1]), "-e", str(edges), "-o", str(tmp_path), "--align", "union"],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--align union needs --sites device" in r.stderr


def test_metaprofile_align_union_equals_the_padded_files(tmp_path):
    from alphabeta_rs_amd import build as B

    B.build_host()
    edges, sides, counts, n_union = tool_inputs(tmp_path)
    base = lambda side: [B.META_CLI, "--methylome", sides[side][0], "--genome", GOLDEN / "annotation.txt", "--nodes",
                         sides[side][1], "--edges", edges, "--iterations", "5", "--seed", "77", "-s", "5", "-w", "5", "-c",
                         "2048", "--sites", "device"]
    hide = [sides["raw"][0], sides["padded"][0], sides["raw"][1], sides["padded"][1]]
    got = run_tool(base("raw") + ["--align", "union"], tmp_path / "out_union", hide)
    want = run_tool(base("padded") + ["--align", "none"], tmp_path / "out_padded", hide)
    assert sorted(got[0]) == sorted(want[0]) and len(want[0]) >= 8 and {"results.txt", "raw.npy", "distributions.txt"} <= set(want[0])
    for name in want[0]:
        assert got[0][name] == want[0][name], name
    assert len(want[0]["results.txt"].splitlines()) > 10
    assert got[1] == want[1] and got[3] == want[3] and not want[2]
    assert "site counts differ" not in got[1]
    assert_union_lines(got[2], counts, n_union)
    r = subprocess.run([str(B.META_CLI), "-o", str(tmp_path), *map(str, base("raw")[1:-2]), "--align", "union"],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--align union needs --sites device" in r.stderr
