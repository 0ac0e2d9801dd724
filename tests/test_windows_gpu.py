"""The device half of the window extraction (abn_windows_*, alphabeta_rs_amd/csrc/abn_windows.hpp) and the in-memory path
of `metaprofile_alphabeta` against the Python restatement of the reference in tests/_windows_model.py.  Every comparison
is exact: integers equal, doubles bit-equal, packed bytes equal to pack_codes of the model's per-window code lists laid
out as layout_packed_call does.  The methylomes are synthesised against tests/golden/annotation.txt (or a two-gene
annotation): the bundled methylomes end before the first gene's upstream region."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import _windows_model as M

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden"


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def methylome(rows):
    """rows of (chromosome, position, strand, status, posterior, level) -> file text with its header row"""
    return M.HEADER + "".join(M.site_line(*r) + "\n" for r in rows)


def window_indices(pairs, args, mgl):
    """the model's windows of one sample as index lists: [w] -> the places of its sites in the file, in push order"""
    return [np.array([x["index"] for x in w], dtype=np.int64) for w in M.flat(M.extract(pairs, args, mgl))]


def check_against_model(abn, ctx, args, mgl, pairs_by_sample, codes_by_sample=None, levels_by_sample=None, shared_idx=None):
    """Create the handle from the model's gene choice and compare everything it reports with the model's windows.
    codes_by_sample / levels_by_sample: samples that share sample 0's coordinates and differ in these arrays only (the
    placement is then modelled once).  Returns (handle, per-sample per-window code arrays, ragged)."""
    counts = M.windows_new(args, mgl)
    off, pos, gs, ge, fl, co, lv = M.soa(pairs_by_sample, args)
    if codes_by_sample is not None:
        n, S = len(codes_by_sample), len(pairs_by_sample[0])
        off = np.arange(n + 1, dtype=np.int64) * S
        pos, gs, ge, fl = (np.tile(a, n) for a in (pos, gs, ge, fl))
        co, lv = np.concatenate(codes_by_sample), np.concatenate(levels_by_sample)
        idx = [shared_idx if shared_idx is not None else window_indices(pairs_by_sample[0], args, mgl)] * n
    else:
        n = len(pairs_by_sample)
        idx = [window_indices(p, args, mgl) for p in pairs_by_sample]
    h = abn.Windows(ctx, off, pos, gs, ge, fl, co, lv, cutoff=args.cutoff, step=args.step, size=args.size,
                    absolute=args.absolute, counts=counts)
    W = sum(counts)
    assert h.W == W and h.n_samples == n
    codes = [[co[off[s] + idx[s][w]] for w in range(W)] for s in range(n)]
    count, ls, lsk, kept = h.stats()
    want_count = np.array([[len(idx[s][w]) for w in range(W)] for s in range(n)], dtype=np.int64).reshape(n, W)
    assert np.array_equal(count, want_count)
    want = np.zeros((3, n, W))
    for s in range(n):
        for w in range(W):                            # the serial folds from 0.0 in push order (np.cumsum adds one by one)
            v = lv[off[s] + idx[s][w]]
            k = v[co[off[s] + idx[s][w]] < 0x80]
            want[:, s, w] = (np.cumsum(v)[-1] if len(v) else 0.0), (np.cumsum(k)[-1] if len(k) else 0.0), len(k)
    assert np.array_equal(bits(ls), bits(want[0])) and np.array_equal(bits(lsk), bits(want[1]))
    assert np.array_equal(kept, want[2].astype(np.int64))
    packed, begin, end, ragged = M.packed_layout_codes(abn, codes)
    b, e, r = h.layout()
    assert np.array_equal(b, begin) and np.array_equal(e, end) and np.array_equal(r, ragged)
    assert h.row_stride == packed.shape[1] and h.n_sites == 4 * packed.shape[1]
    got = h.packed()
    assert got.shape == packed.shape and np.array_equal(got, packed)
    assert h.packed_device_ptr() % 16 == 0
    return h, codes, ragged


TWO_GENES = "1\t1000\t1040\tFORWARD\tx\t+\n1\t2000\t2040\tREVERSE\tx\t-\n"


def boundary_rows():
    """every integer position from start - cutoff - 2 to end + cutoff + 2 of a 40 bp gene on each strand, cutoff 20"""
    return ([(1, p, "+", "M", 0.9999, 0.5) for p in range(1000 - 22, 1040 + 23)] +
            [(1, p, "-", "M", 0.9999, 0.5) for p in range(2000 - 22, 2040 + 23)])


@pytest.mark.parametrize("absolute", [False, True])
@pytest.mark.parametrize("step,size", [(5, 5), (2, 5), (3, 5), (7, 4)])
def test_placement_boundaries(abn, gpu_ctx, absolute, step, size):
    """With step == size a position within 0.1 of a boundary lands in two windows, with step < size a site lands in
    several (step > size leaves gaps).  Five samples share the coordinates; sample k's code of site i is the k-th base-3
    digit of i, so equal packed bytes mean equal index lists."""
    args = M.Args(cutoff=20, step=step, size=size, absolute=absolute)
    genome, genes = M.genome_of(TWO_GENES)
    mgl = M.max_gene_length(genes, absolute)
    pairs = M.choose_genes(methylome(boundary_rows()), genome, args)
    S = len(pairs)
    # without a gene, per gene: start - cutoff - 2 and - 1, and end + cutoff .. + 2 (a site's end is its start + 1)
    assert S == 170 and sum(g is None for _, g in pairs) == 10
    codes = [((np.arange(S) // 3 ** k) % 3).astype(np.uint8) for k in range(5)]
    levels = [np.linspace(0.0, 1.0, S) + k for k in range(5)]
    h, _, ragged = check_against_model(abn, gpu_ctx, args, mgl, [pairs], codes, levels)
    count = h.stats()[0]
    assert not ragged.any() and count.sum() > 0
    if step <= size:
        assert count.sum() > 5 * (S - 10)                           # sites in more than one window
    h.close()


@pytest.fixture(scope="module")
def ranking_case():
    """One gene of 200 bp in absolute mode, step == size == 10, cutoff 50: the gene windows 0..7 hold 0, 1, 15, 16, 17,
    255, 256 and 257 sites (all at the middle of their window), about 70 000 more sites fall on every position of the other
    windows, boundaries included, and the file order is shuffled: memberships of all windows interleave over ~70 blocks."""
    args = M.Args(cutoff=50, step=10, size=10, absolute=True)
    genome, genes = M.genome_of("2\t10000\t10200\tONLY\tx\t+\n")
    rng = np.random.default_rng(20261018)
    where = []
    for w, k in enumerate([0, 1, 15, 16, 17, 255, 256, 257]):
        where += [10000 + 10 * w + 5] * k
    where += list(rng.integers(10081, 10201, size=40000)) + list(rng.integers(9950, 10000, size=15000))
    where += list(rng.integers(10201, 10250, size=14000))
    where = np.array(where)[rng.permutation(len(where))]
    rows = [(2, int(p), "+", "M", 0.9999, 0.5) for p in where]
    pairs = M.choose_genes(methylome(rows), genome, args)
    assert len(pairs) == len(where) > 69000 and all(g is not None for _, g in pairs)
    mgl = M.max_gene_length(genes, True)
    return args, mgl, pairs, window_indices(pairs, args, mgl)


@pytest.mark.parametrize("n", [2, 3, 17])
def test_stable_ranking_and_packing_shapes(abn, gpu_ctx, ranking_case, n):
    args, mgl, pairs, idx = ranking_case
    S = len(pairs)
    rng = np.random.default_rng(n)
    codes = [rng.choice(np.array([0, 1, 2, 0x80, 0x81, 0x82], dtype=np.uint8), size=S, p=[.3, .2, .3, .1, .05, .05])
             for _ in range(n)]
    levels = [rng.random(S) for _ in range(n)]
    h, wcodes, ragged = check_against_model(abn, gpu_ctx, args, mgl, [pairs], codes, levels, idx)
    count = h.stats()[0]
    assert list(count[0, 5:13]) == [0, 1, 15, 16, 17, 255, 256, 257] and not ragged.any()
    b, e, _ = h.layout()
    assert np.all(b % 256 == 0) and list((e - b)[5:13]) == [0, 1, 15, 16, 17, 255, 256, 257]
    diff, both, dval = h.pairwise()
    for w in range(h.W):
        cw = np.array([wcodes[s][w] for s in range(n)], dtype=np.uint8).reshape(n, -1)
        d1, b1, v1 = gpu_ctx.pairwise_divergence(cw)
        assert np.array_equal(diff[w], d1) and np.array_equal(both[w], b1)
        nan = np.isnan(v1)
        assert np.array_equal(np.isnan(dval[w]), nan) and np.array_equal(bits(dval[w][~nan]), bits(v1[~nan]))
    h.close()


def test_sums_follow_the_serial_folds(abn, gpu_ctx):
    """Levels of mixed magnitudes, 1000 and more sites per window: another summation order changes the last bits."""
    args = M.Args(cutoff=200, step=50, size=50, absolute=False)
    genome, genes = M.genome_of("3\t5000\t6000\tONLY\tx\t-\n")
    rng = np.random.default_rng(6)
    rows = [(3, int(p), "-", "UIM"[int(rng.integers(3))], [0.9999, 0.5][int(rng.integers(4) == 0)],
             float(rng.random() * 10.0 ** int(rng.integers(-9, 9)))) for p in rng.integers(4800, 6200, size=6000)]
    pairs = M.choose_genes(methylome(rows), genome, args)
    h, _, _ = check_against_model(abn, gpu_ctx, args, 100, [pairs, pairs[:]])
    count, ls, _, kept = h.stats()
    assert count[0].max() >= 1000 and 0 < kept.sum() < count.sum()
    w = int(np.argmax(count[0]))
    lv = [s["meth_lvl"] for s in M.flat(M.extract(pairs, args, 100))[w]]
    assert float(np.sum(lv)) != ls[0, w] or float(np.sum(lv[::-1])) != ls[0, w]   # the order does matter on this data
    h.close()


def test_ragged_and_empty_windows(abn, gpu_ctx):
    args = M.Args(cutoff=20, step=2, size=5, absolute=False)
    genome, genes = M.genome_of(TWO_GENES)
    rows = boundary_rows()
    full = M.choose_genes(methylome(rows), genome, args)
    gone = 60                                                       # a site inside the first gene
    short = M.choose_genes(methylome(rows[:gone] + rows[gone + 1:]), genome, args)
    h, _, ragged = check_against_model(abn, gpu_ctx, args, 100, [full, short, full])
    counts = M.windows_new(args, 100)
    region, inside = M.place_in_windows(full[gone][0], full[gone][1], args, counts)
    first = [0, counts[0], counts[0] + counts[1]][region]
    assert len(inside) > 1 and sorted(np.flatnonzero(ragged)) == [first + i for i in inside]
    diff, both, dval = h.pairwise()
    assert not both[ragged == 1].any() and np.isnan(dval[ragged == 1]).all() and both[ragged == 0].any()
    h.close()
    # sites that match no gene, and no sites at all: all-zero counts, one super-step of filtered fields per row
    nowhere = M.choose_genes(methylome([(9, p, "+", "M", 0.9999, 0.5) for p in range(900, 1100)]), genome, args)
    assert len(nowhere) == 200
    for case in ([nowhere, nowhere], [[], []], [[]]):
        h, _, ragged = check_against_model(abn, gpu_ctx, args, 100, case)
        assert not h.stats()[0].any() and not ragged.any() and h.row_stride == 64 and np.all(h.packed() == 0xFF)
        if len(case) > 1:
            assert np.isnan(h.pairwise()[2]).all()
        h.close()


def test_bad_arguments_are_status_codes(abn, gpu_ctx):
    z32, z8 = np.zeros(4, dtype=np.uint32), np.zeros(4, dtype=np.uint8)
    for off, step, counts in ([[0, 4], 0, (1, 1, 1)], [[1, 4], 5, (1, 1, 1)], [[0, 6, 4], 5, (1, 1, 1)], [[0, 4], 5, (1, -1, 1)]):
        with pytest.raises(abn.AbnError) as err:
            abn.Windows(gpu_ctx, off, z32, z32, z32, z8, z8, np.zeros(4), cutoff=10, step=step, size=5, absolute=False,
                        counts=counts)
        assert err.value.status == 1


def test_metaprofile_in_memory_equals_the_directory_path(abn, tmp_path):
    """Synthetic methylomes of the bundled 4-sample pedigree over the first genes of the annotation: `metaprofile_alphabeta
    --methylome ..` writes the raw.npy bytes and the results.txt of `metaprofile_alphabeta -o tree` on the directory tree the
    model writes as src/setup.rs and Windows::save would, and the model's four kinds of side files."""
    from alphabeta_rs_amd import build as B

    B.build_host()
    annotation = (GOLDEN / "annotation.txt").read_text()
    args = M.Args(cutoff=2048, step=5, size=5, absolute=False)
    genome, genes = M.genome_of(annotation)
    rng = np.random.default_rng(8)
    where = []
    for g in sorted(genes, key=lambda g: (g["chromosome"], g["start"]))[:3]:
        where += [(g, int(p)) for p in sorted(rng.integers(g["start"] - 2100, g["end"] + 2100, size=1000))]
    names = ["G0.txt", "G1_2.txt", "G4_2.txt", "G4_8.txt"]
    meth = tmp_path / "methylome"
    meth.mkdir()
    status = rng.choice([0, 2], size=len(where), p=[0.6, 0.4])
    texts = {}
    for k, name in enumerate(names):
        if k:
            flip = rng.random(len(where)) < 0.04 * k
            status = np.where(flip, rng.integers(0, 3, size=len(where)), status)
        rows = [(g["chromosome"], p, "+-*"[g["strand"]].replace("*", "+"), "UIM"[int(s)], [0.9999, 0.7][int(rng.integers(10) == 0)],
                 round(float(0.05 + 0.45 * s + 0.04 * rng.random()), 4)) for (g, p), s in zip(where, status)]
        texts[name] = methylome(rows)
        (meth / name).write_text(texts[name])
    nodes = "filename\tnode\tgen\tmeth\n" + "".join(
        f"{meth}/{f}\t{node}\t{gen}\t{m}\n" for f, node, gen, m in
        [("G0.txt", "0_0", 0, "Y"), ("G1_2.txt", "1_2", 1, "Y"), ("G1_8.txt", "1_8", 1, "N"), ("G2_2.txt", "2_2", 2, "N"),
         ("G2_8.txt", "2_8", 2, "N")]) + "-\t3_2\t3\tN\n-\t3_8\t3\tN\n" + f"{meth}/G4_2.txt\t4_2\t4\tY\n{meth}/G4_8.txt\t4_8\t4\tY\n"
    edges = (GOLDEN / "data" / "edgelist.txt").read_text()
    (tmp_path / "nodelist.fn").write_text(nodes)
    (tmp_path / "edgelist.fn").write_text(edges)
    wins = {n: M.extract(M.choose_genes(texts[n], genome, args), args, 100) for n in names}
    tree, out = tmp_path / "tree", tmp_path / "out"
    tree.mkdir()
    out.mkdir()
    M.save_tree(tree, args, 100, nodes, edges, wins)
    dist = [len(w) for w in M.flat(wins[names[0]])]
    (tmp_path / "dist.txt").write_text("".join(f"{c}\n" for c in dist))
    common = ["--iterations", "20", "--seed", "77", "-s", "5", "-w", "5", "-c", "2048"]
    r1 = subprocess.run([str(B.META_CLI), "-o", str(tree), "--distribution", str(tmp_path / "dist.txt"), *common],
                        capture_output=True, text=True, timeout=300)
    assert r1.returncode == 0, r1.stdout[-2000:] + r1.stderr[-2000:]
    r2 = subprocess.run([str(B.META_CLI), "-o", str(out), "--methylome", str(meth), "--genome", str(GOLDEN / "annotation.txt"),
                         "--nodes", str(tmp_path / "nodelist.fn"), "--edges", str(tmp_path / "edgelist.fn"), *common],
                        capture_output=True, text=True, timeout=300)
    assert r2.returncode == 0, r2.stdout[-2000:] + r2.stderr[-2000:]
    assert (out / "raw.npy").read_bytes() == (tree / "raw.npy").read_bytes()
    res = (out / "results.txt").read_text()
    assert res == (tree / "results.txt").read_text()
    lines = res.splitlines()[1:]
    assert len(lines) >= 50 and np.load(out / "raw.npy").shape == (20, 7, len(lines))
    assert [int(l.split(";")[2]) for l in lines] == dist[:len(lines)] and min(dist) > 0      # real counts in cg_count
    for name, text in M.side_files(names, wins).items():
        assert (out / name).read_text() == text, name
    # --invert is refused by the new path, and the new flags belong to it
    r3 = subprocess.run([str(B.META_CLI), "-o", str(out), "--methylome", str(meth), "--genome", "x", "--nodes", "x",
                         "--edges", "x", "--invert"], capture_output=True, text=True, timeout=60)
    assert r3.returncode == 2 and "--invert is not supported" in r3.stderr
