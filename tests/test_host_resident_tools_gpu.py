"""What the three drivers of the host layer that start from resident methylomes print and write, pinned from outside: the
whole stdout of `metaprofile_alphabeta --methylome` (its per-window refusals and their order), of the same tool and of
`--tiles` on a graph whose shortest paths contradict the generation times, the three per-tile refusals of `--regions`, and
the per-sample lines of `--align position | union` of both tools.  Every expected text is built here from the inputs; every
run is a child process on three or four methylomes of a few hundred sites."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import _windows_model as M

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden"
NAMES = ["G0.txt", "G1_2.txt", "G4_2.txt", "G4_8.txt"]      # the bundled pedigree's sampled nodes, in nodelist order
ANNOTATION = "1\t10000\t11000\tONLY\tx\t+\n"
CUTOFF, GONE = 500, 140                                     # site GONE of NAMES[2] is missing in "short": inside the gene
BUILDING = "Error: Error while building pedigree: "
PATH_LENGTH = "path length does not match the generation times"


def run(exe, *args):
    return subprocess.run([str(exe), *map(str, args)], capture_output=True, text=True, timeout=300)


def drifting(rng, n):
    """the statuses of the four samples at n sites: the later generations drift from the founder's"""
    status = rng.choice([0, 2], size=n, p=[0.6, 0.4])
    out = []
    for k in range(len(NAMES)):
        if k:
            status = np.where(rng.random(n) < 0.04 * k, rng.integers(0, 3, size=n), status)
        out.append(status.copy())
    return out


def lines_of(rng, positions, status, posterior=None):
    return [M.site_line(1, p, "+", "UIM"[int(s)], posterior or [0.9999, 0.7][int(rng.integers(10) == 0)],
                        round(float(0.05 + 0.45 * s + 0.04 * rng.random()), 4)) for p, s in zip(positions, status)]


def write_methylomes(meth, lines_by_name):
    meth.mkdir()
    for name, lines in lines_by_name.items():
        (meth / name).write_text(M.HEADER + "".join(l + "\n" for l in lines))


def bundled_graph(d, meth):
    """the bundled nodelist with the sampled nodes' files in `meth`, and the bundled edgelist -> (nodes text, edges text)"""
    nodes = "filename\tnode\tgen\tmeth\n" + "".join(
        f"{meth}/{f}\t{node}\t{gen}\t{m}\n" for f, node, gen, m in
        [("G0.txt", "0_0", 0, "Y"), ("G1_2.txt", "1_2", 1, "Y"), ("G1_8.txt", "1_8", 1, "N"), ("G2_2.txt", "2_2", 2, "N"),
         ("G2_8.txt", "2_8", 2, "N")]) + "-\t3_2\t3\tN\n-\t3_8\t3\tN\n" + f"{meth}/G4_2.txt\t4_2\t4\tY\n{meth}/G4_8.txt\t4_8\t4\tY\n"
    edges = (GOLDEN / "data" / "edgelist.txt").read_text()
    (d / "nodelist.fn").write_text(nodes)
    (d / "edgelist.fn").write_text(edges)
    return nodes, edges


def chain_graph(d, meth):
    """a - b - c - d, all sampled, generations 0, 2, 1, 3: the path a .. c weighs 3 where the rule gives 1"""
    (d / "chain_nodes.fn").write_text("filename\tnode\tgen\tmeth\n" + "".join(
        f"{meth}/{f}\t{node}\t{gen}\tY\n" for f, node, gen in zip(NAMES, "abcd", (0, 2, 1, 3))))
    (d / "chain_edges.fn").write_text("from\tto\tgendiff\na\tb\t2\nb\tc\t1\nc\td\t2\n")
    return ["--nodes", d / "chain_nodes.fn", "--edges", d / "chain_edges.fn"]


@pytest.fixture(scope="module")
def gene_case(tmp_path_factory):
    """286 sites from 500 bp before a 1000 bp gene to 500 bp behind it, in four methylomes: "full" holds every site in
    every sample, "short" lacks site GONE in the third"""
    from alphabeta_rs_amd import build as B

    B.build_host()
    d = tmp_path_factory.mktemp("gene_case")
    rng = np.random.default_rng(11)
    positions = list(range(9500, 11500, 7))
    status = drifting(rng, len(positions))
    lines = {name: lines_of(rng, positions, s) for name, s in zip(NAMES, status)}
    write_methylomes(d / "full", lines)
    write_methylomes(d / "short", {n: l[:GONE] + l[GONE + 1:] if n == NAMES[2] else l for n, l in lines.items()})
    (d / "annotation.txt").write_text(ANNOTATION)
    return B, d


def window_errors(out, args, wins, healthy=None):
    """the stdout lines of alphabeta_multiple_in_memory's window loop, in the (region, window) enumeration's order: a window
    it names beyond those created, a ragged one with its pairs' lines, and `healthy` (a text or None) at every other"""
    counts = M.windows_new(args, 100)
    lines, failed = [], []
    for r, region in enumerate(M.REGIONS):
        for k, window in enumerate(range(0, 100, args.step)):
            if k >= counts[r]:
                lines.append(f"{BUILDING}Could not open node file: {out}/{region}/{window}/{NAMES[0]}")
                continue
            c = [len(wins[name][r][k]) for name in NAMES]
            if len(set(c)) > 1:
                lines += [f"Lengths do not match, all bets are off: {c[a]} vs {c[b]}"
                          for a in range(len(c)) for b in range(a + 1, len(c)) if c[a] != c[b]]
                lines.append(f"{BUILDING}the samples' site counts differ in this window")
                failed.append((region, window))
            elif healthy:
                lines.append(BUILDING + healthy)
    return lines, failed


def model_windows(d, side, args):
    genome, _ = M.genome_of(ANNOTATION)
    return {n: M.extract(M.choose_genes((d / side / n).read_text(), genome, args), args, 100) for n in NAMES}


def test_metaprofile_methylome_stdout_and_files(gene_case, tmp_path):
    """-s 30 -w 30: the enumeration names window 90 of every region, which Windows::new does not create; the window that
    holds site GONE is ragged.  The whole stdout; results.txt and raw.npy of the directory path on a tree in which the
    ragged window cannot be read either."""
    B, d = gene_case
    args = M.Args(cutoff=CUTOFF, step=30, size=30, absolute=False)
    wins = model_windows(d, "short", args)
    nodes, edges = bundled_graph(tmp_path, d / "short")
    tree, out = tmp_path / "tree", tmp_path / "out"
    tree.mkdir(), out.mkdir()
    errors, failed = window_errors(out, args, wins)
    assert len(failed) == 1 and sum("Could not open" in l for l in errors) == 3 and sum("Lengths" in l for l in errors) == 3
    M.save_tree(tree, args, 100, nodes, edges, wins)
    for region, window in failed:
        (tree / region / str(window) / NAMES[0]).unlink()
    dist = [len(w) for w in M.flat(wins[NAMES[0]])]
    (tmp_path / "dist.txt").write_text("".join(f"{c}\n" for c in dist))
    common = ["--iterations", "5", "--seed", "77", "-s", "30", "-w", "30", "-c", CUTOFF]
    r1 = run(B.META_CLI, "-o", tree, "--distribution", tmp_path / "dist.txt", *common)
    assert r1.returncode == 0, r1.stdout[-2000:] + r1.stderr[-2000:]
    r2 = run(B.META_CLI, "-o", out, "--methylome", d / "short", "--genome", d / "annotation.txt", "--nodes",
             tmp_path / "nodelist.fn", "--edges", tmp_path / "edgelist.fn", *common)
    assert r2.returncode == 0, r2.stdout[-2000:] + r2.stderr[-2000:]
    res = (out / "results.txt").read_text()
    print(r2.stdout)
    assert r2.stdout == "".join(l + "\n" for l in ["Starting run Anonymous Run"] + errors) + res + "\n"
    assert res == (tree / "results.txt").read_text() and len(res.splitlines()) == 1 + 8
    assert (out / "raw.npy").read_bytes() == (tree / "raw.npy").read_bytes()
    assert np.load(out / "raw.npy").shape == (5, 7, 8)


def test_metaprofile_methylome_on_an_inconsistent_graph(gene_case, tmp_path):
    """DMatrix::convert refuses the graph itself: every enumerated window reports it and the run ends with an empty result;
    a window that fails before the conversion keeps its own text"""
    B, d = gene_case
    graph = chain_graph(tmp_path, d / "full")
    base = ["--genome", d / "annotation.txt", *graph, "--iterations", "4", "--seed", "77", "-c", CUTOFF]
    out = tmp_path / "out"
    out.mkdir()
    r = run(B.META_CLI, "-o", out, "--methylome", d / "full", *base, "-s", "50", "-w", "50")
    print(r.stdout)
    assert r.returncode == 0 and r.stdout == "Starting run Anonymous Run\n" + f"{BUILDING}{PATH_LENGTH}\n" * 6 + "\n"
    assert (out / "results.txt").read_text() == "" and np.load(out / "raw.npy").shape == (4, 7, 0)
    args = M.Args(cutoff=CUTOFF, step=30, size=30, absolute=False)
    out2 = tmp_path / "out2"
    out2.mkdir()
    errors, failed = window_errors(out2, args, model_windows(d, "short", args), healthy=PATH_LENGTH)
    assert len(failed) == 1 and len(errors) == 12 + 3 and sum(PATH_LENGTH in l for l in errors) == 8
    r = run(B.META_CLI, "-o", out2, "--methylome", d / "short", *base, "-s", "30", "-w", "30")
    print(r.stdout)
    assert r.returncode == 0 and r.stdout == "".join(l + "\n" for l in ["Starting run Anonymous Run"] + errors) + "\n"
    assert (out2 / "results.txt").read_text() == "" and np.load(out2 / "raw.npy").shape == (4, 7, 0)


def test_metaprofile_tiles_on_an_inconsistent_graph(gene_case, tmp_path):
    """the tiles driver converts the graph once, in front of its tiles: the refusal ends the run"""
    B, d = gene_case
    r = run(B.META_CLI, "-o", tmp_path, "--methylome", d / "full", *chain_graph(tmp_path, d / "full"), "--tiles", "500",
            "--iterations", "4", "--seed", "77")
    print(r.stdout, r.stderr)
    assert r.returncode == 1 and r.stdout == f"Starting run Anonymous Run\nError: {PATH_LENGTH}\n" and r.stderr == ""
    assert not (tmp_path / "results.txt").exists() and not (tmp_path / "tiles.txt").exists()


def test_metaprofile_regions_refusals(gene_case, tmp_path):
    """--regions --align union over five tiles: a healthy one, one without a site, one in which the second sample keeps no
    site above the filter, one in which the first two samples hold disjoint sites, a healthy one"""
    B, _ = gene_case
    rng = np.random.default_rng(12)
    positions = [10 * i + 5 for i in range(400)]
    status = drifting(rng, len(positions))
    lines = {}
    for k, name in enumerate(NAMES):                        # 100 sites per 1000 bp, all above the filter, but:
        mine = lines_of(rng, positions, status[k], posterior=0.9999)
        if k == 1:                                          # 1:1000-2000: every site of the second sample below it
            mine[100:200] = lines_of(rng, positions[100:200], status[k][100:200], posterior=0.7)
        if k < 2:                                           # 1:2000-3000: the first sample lacks the odd sites, the second the even
            mine = [l for i, l in enumerate(mine) if not (200 <= i < 300 and i % 2 != k)]
        lines[name] = mine
    meth = tmp_path / "methylome"
    write_methylomes(meth, lines)
    bundled_graph(tmp_path, meth)
    (tmp_path / "regions.bed").write_text("chr1\t0\t1000\nchr3\t0\t1000\nchr1\t1000\t2000\nchr1\t2000\t3000\nchr1\t3000\t4000\n")
    r = run(B.META_CLI, "-o", tmp_path, "--methylome", meth, "--nodes", tmp_path / "nodelist.fn", "--edges",
            tmp_path / "edgelist.fn", "--regions", tmp_path / "regions.bed", "--align", "union", "--iterations", "5", "--seed", "77")
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    want = ["Starting run Anonymous Run"]
    want += [f"Aligned by union: {name}: {len(lines[name])} sites, 400 in the union" for name in NAMES]
    assert [len(lines[name]) for name in NAMES] == [350, 350, 400, 400]
    want += [f"{BUILDING}tile 1 (3:0-1000): no site lies in this tile",
             f"{BUILDING}tile 2 (1:1000-2000): {NAMES[1]} has no site above the posterior filter in this tile",
             f"{BUILDING}tile 3 (1:2000-3000): {NAMES[0]} and {NAMES[1]} share no site above the posterior filter in this tile"]
    res = (tmp_path / "results.txt").read_text()
    assert r.stdout == "".join(l + "\n" for l in want) + res + "\n"
    assert [l.split(";")[1] for l in res.splitlines()[1:]] == ["0", "4"]
    assert (tmp_path / "tiles.txt").read_text() == ("tile;chromosome;start;end;cg_count;fitted\n0;1;0;1000;100;1\n1;3;0;1000;0;0\n"
                                                    "2;1;1000;2000;100;0\n3;1;2000;3000;100;0\n4;1;3000;4000;100;1\n")


@pytest.fixture(scope="module")
def lacking_case(gene_case, tmp_path_factory):
    """the sites of gene_case in three methylomes, each lacking five sites of its own -> (B, annotation, directory, nodelist,
    edgelist, names, sites per file, sites all share, sites any holds)"""
    B, g = gene_case
    d = tmp_path_factory.mktemp("lacking_case")
    rng = np.random.default_rng(13)
    positions = list(range(9500, 11500, 7))
    names = [NAMES[0], NAMES[2], NAMES[3]]
    status = drifting(rng, len(positions))
    gone = [set(range(20 + k, len(positions), 60)) for k in range(3)]
    assert all(len(x) == 5 for x in gone) and not (gone[0] & gone[1]) and not (gone[1] & gone[2])
    lines = {name: [l for i, l in enumerate(lines_of(rng, positions, s)) if i not in x]
             for name, s, x in zip(names, (status[0], status[2], status[3]), gone)}
    meth = d / "methylome"
    write_methylomes(meth, lines)
    (d / "nodelist.fn").write_text("filename\tnode\tgen\tmeth\n" + "".join(
        f"{f}\t{node}\t{gen}\t{m}\n" for f, node, gen, m in
        [(f"{meth}/G0.txt", "0_0", 0, "Y"), ("-", "1_2", 1, "N"), ("-", "1_8", 1, "N"), ("-", "2_2", 2, "N"), ("-", "2_8", 2, "N"),
         ("-", "3_2", 3, "N"), ("-", "3_8", 3, "N"), (f"{meth}/G4_2.txt", "4_2", 4, "Y"), (f"{meth}/G4_8.txt", "4_8", 4, "Y")]))
    (d / "edgelist.fn").write_text((GOLDEN / "data" / "edgelist.txt").read_text())
    n = len(positions)
    return B, g / "annotation.txt", meth, d / "nodelist.fn", d / "edgelist.fn", names, [n - 5] * 3, n - 15, n


def aligned_lines(align, shown, counts, n_common, n_union):
    if align == "position":
        return [f"Aligned by position: {name}: {c} sites, {n_common} kept" for name, c in zip(shown, counts)]
    return [f"Aligned by union: {name}: {c} sites, {n_union} in the union" for name, c in zip(shown, counts)]


@pytest.mark.parametrize("align", ["position", "union"])
def test_alphabeta_sites_device_reports_every_sample(lacking_case, tmp_path, align):
    """`alphabeta --sites device --align ..`: one line per sampled node, named as the nodelist names its file"""
    B, _, meth, nodes, edges, names, counts, n_common, n_union = lacking_case
    r = run(B.CLI, "-i", "5", "-n", nodes, "-e", edges, "--parse", "device", "--sites", "device", "--align", align, "-o", tmp_path)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = r.stdout.splitlines()
    at = out.index("Building pedigree...")
    assert out[at + 1:at + 4] == aligned_lines(align, [f"{meth}/{n}" for n in names], counts, n_common, n_union)
    assert sum(l.startswith("Aligned by") for l in out) == 3 and "Lengths do not match" not in r.stdout


@pytest.mark.parametrize("align", ["position", "union"])
def test_metaprofile_sites_device_reports_every_sample(lacking_case, tmp_path, align):
    """`metaprofile_alphabeta --methylome .. --sites device --align ..`: one line per methylome file, by its name, in front of
    the windows' lines"""
    B, annotation, meth, nodes, edges, names, counts, n_common, n_union = lacking_case
    r = run(B.META_CLI, "-o", tmp_path, "--methylome", meth, "--genome", annotation, "--nodes", nodes, "--edges", edges,
            "--iterations", "5", "--seed", "77", "-s", "50", "-w", "50", "-c", CUTOFF, "--sites", "device", "--align", align)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.splitlines()[:4] == ["Starting run Anonymous Run"] + aligned_lines(align, names, counts, n_common, n_union)
    assert sum(l.startswith("Aligned by") for l in r.stdout.splitlines()) == 3 and "Lengths do not match" not in r.stdout
    assert r.stdout.endswith((tmp_path / "results.txt").read_text() + "\n")
