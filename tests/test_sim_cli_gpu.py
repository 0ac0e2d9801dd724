"""`alphabeta --simulate`: the pedigree it writes equals alphabeta_rs_amd.simulate.pedigree for the same arguments, bit for
bit; the flag combinations it refuses, by their messages; and a run without the flag writes what the untouched paths write."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import _sim_model as M
from alphabeta_rs_amd import simulate as S

pytestmark = pytest.mark.gpu
GOLDEN = Path(__file__).resolve().parent / "golden"        # data/nodelist.txt and data/edgelist.txt are a tree: 0_0 its root
LISTS = ("-n", "data/nodelist.txt", "-e", "data/edgelist.txt")


def alphabeta(*args, timeout=120):
    from alphabeta_rs_amd import build as B

    B.build_host()
    return subprocess.run([str(B.CLI), *map(str, args)], capture_output=True, text=True, timeout=timeout, cwd=GOLDEN)


def golden_tree():
    nodes = []
    for line in (GOLDEN / "data" / "nodelist.txt").read_text().splitlines()[1:]:
        f = line.split(",")
        if len(f) >= 4:
            nodes.append((f[1], int(f[2]), f[3] == "Y"))
    edges = [tuple(line.split("\t")[:2]) for line in (GOLDEN / "data" / "edgelist.txt").read_text().splitlines()[1:] if "\t" in line]
    return M.breadth_first(nodes, edges)


def written_pedigree(path):
    lines = path.read_text().splitlines()
    assert lines[0] == "time0\ttime1\ttime2\tD.value"
    return np.array([[float(x) for x in line.split("\t")] for line in lines[1:]]).reshape(-1, 4)


def test_simulated_run_writes_the_pedigree_of_the_binding(gpu_ctx, oracle, tmp_path):
    parent, generation, emit = golden_tree()
    assert parent == [-1, 0, 0, 1, 2, 3, 4, 5, 6] and generation == [0, 1, 1, 1, 1, 3, 3, 4, 4] and emit == [1, 1, 0, 0, 0, 0, 0, 1, 1]
    seed, L = 77, 200_000
    r = alphabeta("--simulate", "2e-3,5e-3", "--sim-sites", L, "--seed", seed, "-i", 20, *LISTS, "-o", tmp_path)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "Simulating pedigree..." in r.stdout and "Building pedigree" not in r.stdout
    assert {p.name for p in tmp_path.iterdir()} >= {"pedigree.txt", "analysis.txt", "raw.npy"}
    rows, p0uu = S.pedigree(gpu_ctx, seed, parent, generation, emit, 2e-3, 5e-3, 0.75, 0.5, L)          # the defaults of the tool
    assert np.array_equal(written_pedigree(tmp_path / "pedigree.txt"), rows)
    assert f"Observed steady state methylation {np.format_float_positional(1.0 - p0uu, unique=True, trim='-')}" in r.stdout
    thr = S.thresholds(parent, generation, 2e-3, 5e-3, 0.75, 0.5)
    want_rows, want_p0uu, _, _ = M.pedigree(M.states(seed, parent, thr.tolist(), L), parent, generation, emit)
    assert np.array_equal(rows, want_rows) and p0uu == want_p0uu
    dt, _ = oracle.divergence(rows, 0.25, 0.75, 2e-3, 5e-3, 0.5)
    assert (np.abs(rows[:, 3] - dt) <= 6.0 * np.sqrt(dt / L)).all()
    out = tmp_path / "other"
    out.mkdir()
    r = alphabeta("--simulate=1e-3,1e-3", "--sim-sites", 5000, "--sim-p0uu", 0.6, "--sim-weight", 0.2, "-i", 20, *LISTS, "-o", out)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    rows, _ = S.pedigree(gpu_ctx, 20260101, parent, generation, emit, 1e-3, 1e-3, 0.6, 0.2, 5000)
    assert np.array_equal(written_pedigree(out / "pedigree.txt"), rows)


def test_refused_combinations(tmp_path):
    sim = ("--simulate", "2e-3,5e-3", "--sim-sites", 1000, *LISTS, "-o", tmp_path)
    for extra, words in ((("--sites", "device"), "--simulate cannot be combined with --sites"),
                         (("--parse", "device"), "--simulate cannot be combined with --parse"),
                         (("--contexts", "CG"), "--simulate cannot be combined with --contexts"),
                         (("--sort",), "--simulate cannot be combined with --sort"),
                         (("--dedup", "first"), "--simulate cannot be combined with --dedup"),
                         (("--align", "position"), "--simulate cannot be combined with --align"),
                         (("--pedigree", "pedigree.txt", "--p0uu", "0.5"), "--simulate cannot be combined with --pedigree"),
                         (("--transitions",), "--simulate cannot be combined with --transitions")):
        r = alphabeta(*sim, *extra)
        assert r.returncode == 2 and words in r.stderr, (extra, r.stderr)
    r = alphabeta("--simulate", "2e-3,5e-3", *LISTS, "-o", tmp_path)
    assert r.returncode == 2 and "--simulate needs --sim-sites" in r.stderr
    r = alphabeta("--simulate", "2e-3", "--sim-sites", 1000, *LISTS, "-o", tmp_path)
    assert r.returncode == 2 and "--simulate expects ALPHA,BETA" in r.stderr
    r = alphabeta("--sim-sites", 1000, *LISTS, "-o", tmp_path)
    assert r.returncode == 2 and "belong to --simulate" in r.stderr
    r = alphabeta("--simulate", "2,5e-3", "--sim-sites", 1000, *LISTS, "-o", tmp_path)
    assert r.returncode == 1 and "lie in [0, 1]" in r.stdout
    assert not list(tmp_path.iterdir())
    # an edgelist that is no tree over the nodelist: two roots; a node with two incoming edges; a cycle apart from the root
    nodes = "filename,node,gen,meth\n-,a,0,Y\n-,b,1,Y\n-,c,2,Y\n-,d,2,N\n"
    for edges, words in (("a\tb\nc\td\n", "both have no incoming edge"), ("a\tb\na\tc\nb\td\nc\td\n", "more than one incoming edge"),
                         ("a\tb\nc\td\nd\tc\n", "a cycle apart from the root's tree"), ("a\tb\nb\tc\nc\ta\na\td\n", "no node without an incoming edge")):
        (tmp_path / "nodes.txt").write_text(nodes)
        (tmp_path / "edges.txt").write_text("from\tto\n" + edges)
        out = tmp_path / "out"
        out.mkdir(exist_ok=True)
        r = alphabeta("--simulate", "2e-3,5e-3", "--sim-sites", 1000, "-n", tmp_path / "nodes.txt", "-e", tmp_path / "edges.txt", "-o", out)
        assert r.returncode == 1 and words in r.stdout, (edges, r.stdout)


def test_a_run_without_the_flag_is_unchanged(golden, tmp_path):
    """The default run builds the golden pedigree from the methylome files; its fit's files are the bytes of the run that
    starts from that pedigree file (--pedigree, a path the simulation does not touch)."""
    a, b = tmp_path / "a", tmp_path / "b"
    a.mkdir(), b.mkdir()
    r = alphabeta("-i", 20, *LISTS, "-o", a)
    assert r.returncode == 0 and "Simulating" not in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    assert np.array_equal(written_pedigree(a / "pedigree.txt"), golden["generated"])
    r = alphabeta("-i", 20, "--pedigree", "pedigree_generated.txt", "--p0uu", repr(golden["p0uu_generated"]), "-o", b)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    for name in ("pedigree.txt", "analysis.txt", "raw.npy"):
        assert (a / name).read_bytes() == (b / name).read_bytes(), name
