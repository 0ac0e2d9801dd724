"""`metaprofile_alphabeta --block-bootstrap R [--block-starts S]` (alphabeta_rs_amd/host/block_bootstrap.hpp): every alpha and
beta behind block_bootstrap.txt and block_raw.npy against a Plan built here from Tiles.block_bootstrap's outputs with the
stated window ids, the sd and CI columns against analyze() of those rows, the other output files byte for byte against the
run without the flag, the one `genome` group of --tiles, and the refusals of the flag."""
import ctypes as C

import numpy as np
import pytest

import _parse_model as P
from test_tiles_gpu import NAMES, N_TILES, TILE, graph_files, resident, run_cli, tool_methylomes

pytestmark = pytest.mark.gpu
R, S, SEED, FILTER = 8, 2, 77, 0.99
IDENTITY = (1 << 20) - 1
HEADER = ("group;name;blocks;replicates;replicates_ok;alpha;beta;sd_alpha;sd_beta;ci_alpha_0.025;ci_alpha_0.975;ci_beta_0.025;"
          "ci_beta_0.975")


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    """the methylomes, the graph, a region list of two pools (the even and the odd 1000-bp bins: six segments each, every
    one with sites of every pair) and the two runs on it, without and with the flag"""
    tmp = tmp_path_factory.mktemp("blocks_cli")
    meth = tmp / "methylome"
    tool_methylomes(meth)
    graph_files(tmp, meth)
    (tmp / "regions.bed").write_text("".join(f"chr1\t{TILE * k}\t{TILE * (k + 1)}\t{'even' if k % 2 == 0 else 'odd'}\n"
                                             for k in range(N_TILES)))
    graph = ["--methylome", meth, "--nodes", tmp / "nodelist.fn", "--edges", tmp / "edgelist.fn", "--iterations", "20",
             "--seed", SEED]
    plain, flagged = tmp / "plain", tmp / "flagged"
    plain.mkdir(), flagged.mkdir()
    r0 = run_cli("-o", plain, *graph, "--regions", tmp / "regions.bed", "--pool")
    assert r0.returncode == 0, r0.stdout[-2000:] + r0.stderr[-2000:]
    r1 = run_cli("-o", flagged, *graph, "--regions", tmp / "regions.bed", "--pool", "--block-bootstrap", R, "--block-starts", S)
    assert r1.returncode == 0, r1.stdout[-2000:] + r1.stderr[-2000:]
    return {"tmp": tmp, "meth": meth, "graph": graph, "plain": plain, "flagged": flagged}


def table(path):
    lines = path.read_text().splitlines()
    assert lines[0] == HEADER
    return [l.split(";") for l in lines[1:]]


def test_the_other_files_do_not_change(run):
    for name in ("results.txt", "raw.npy", "pools.txt"):
        assert (run["flagged"] / name).read_bytes() == (run["plain"] / name).read_bytes(), name
    assert not (run["plain"] / "block_bootstrap.txt").exists() and not (run["plain"] / "block_raw.npy").exists()


def test_every_replicate_is_fitted(run):
    rows = table(run["flagged"] / "block_bootstrap.txt")
    assert [r[:5] for r in rows] == [["0", "even", "6", str(R), str(R)], ["1", "odd", "6", str(R), str(R)]]
    raw = np.load(run["flagged"] / "block_raw.npy")
    assert raw.shape == (R, 7, 2) and raw.dtype == np.float64 and np.isfinite(raw).all()


def pedigree_of_the_graph(L, run, whole_dvalue):
    """the generations of the pedigree's rows and every row's pair of samples: Pedigree::build on the whole methylomes, its
    D column matched against the whole-genome D of every pair"""
    rows, p0, err = np.zeros((64, 4)), C.c_double(), C.create_string_buffer(512)
    L.abh_pedigree_build.argtypes = [C.c_char_p, C.c_char_p, C.c_double, C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_double),
                                     C.c_char_p, C.c_int]
    n = L.abh_pedigree_build(str(run["tmp"] / "nodelist.fn").encode(), str(run["tmp"] / "edgelist.fn").encode(), FILTER,
                             rows.ctypes.data_as(C.POINTER(C.c_double)), 64, C.byref(p0), err, 512)
    assert n > 0, err.value
    pair = [int(np.argmin(np.abs(whole_dvalue - d))) for d in rows[:n, 3]]
    assert sorted(pair) == sorted(set(pair)) and np.allclose(whole_dvalue[pair], rows[:n, 3], rtol=1e-12, atol=0)
    return rows[:n, :3].copy(), pair


def test_rates_equal_a_plan_built_from_the_handle(abn, gpu_ctx, run):
    L = P.hostlib()
    sites = [resident(gpu_ctx, L, (run["meth"] / name).read_bytes()) for name in NAMES]
    tiles = abn.Tiles.from_parsed(gpu_ctx, sites, posterior_max_filter=FILTER)
    try:
        tiles.set_fixed(1 << 32)
        gens, pair = pedigree_of_the_graph(L, run, tiles.pairwise()[2][0])
        k = np.arange(N_TILES)
        tiles.set_pools(np.ones(N_TILES, dtype=np.int32), TILE * k, TILE * (k + 1), k % 2, 2)
        out = tiles.block_bootstrap(SEED, R)
        assert (out["both"] > 0).all() and (out["kept"] > 0).all()
        G, rows, n = out["level"].shape
        d_obs, p0uu, ids = [], [], []
        for g in range(G):
            for r in range(rows):
                p0 = 0.0
                for a in range(n):
                    p0 += 1.0 - out["level"][g, r, a] / float(out["kept"][g, r, a])
                p0uu.append(p0 / float(n))
                d_obs.append(out["dvalue"][g, r, pair])
                ids.append((g << 20) | (IDENTITY if r == R else r))
        plan = abn.Plan(gpu_ctx, gens, G * rows, S, 0, options=abn.default_options(seed=SEED))
        try:
            plan.set_window_ids(ids)
            plan.set_windows(np.array(d_obs), np.array(p0uu))
            plan.run()
            models = plan.download()["models"].reshape(G, rows, 4)
        finally:
            plan.close()
    finally:
        tiles.close()
        for s in sites:
            s.close()
    got = table(run["flagged"] / "block_bootstrap.txt")
    raw = np.load(run["flagged"] / "block_raw.npy")
    for g in range(G):
        assert [float(v) for v in got[g][5:7]] == models[g, R, :2].tolist()     # alpha and beta: the identity row's
        want = gpu_ctx.bootstrap_rows(models[g, :R])
        assert raw[:, :, g].tobytes() == want.tobytes()
        a = abn.analyze(want)
        assert [float(v) for v in got[g][7:]] == [a[1, 0], a[1, 1], a[2, 0], a[3, 0], a[2, 1], a[3, 1]]
    assert models[0, R, 0] != models[1, R, 0] and len({m[0] for m in models[0, :R]}) > 1


def test_tiles_write_one_genome_group(run):
    out = run["tmp"] / "tiled"
    out.mkdir()
    r = run_cli("-o", out, *run["graph"], "--tiles", TILE, "--block-bootstrap", R)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    rows = table(out / "block_bootstrap.txt")
    assert len(rows) == 1 and rows[0][:4] == ["0", "genome", str(N_TILES), str(R)] and rows[0][4] == str(R)
    assert np.load(out / "block_raw.npy").shape == (R, 7, 1) and all(np.isfinite(float(v)) for v in rows[0][5:])


def test_the_flag_is_refused_elsewhere(run):
    tmp, graph = run["tmp"], run["graph"]
    for extra, words in ((["--regions", tmp / "regions.bed", "--block-bootstrap", 8], "needs --pool"),
                         (["--tiles", 1000, "--tile-step", 500, "--block-bootstrap", 8], "do not overlap"),
                         (["--tiles", 1000, "--block-bootstrap", 8, "--devices", "0,1"], "one device"),
                         (["--tiles", 1000, "--block-starts", 3], "belongs to --block-bootstrap"),
                         (["--tiles", 1000, "--block-bootstrap", 0], "--block-bootstrap expects"),
                         (["--tiles", 1000, "--block-bootstrap", 1 << 20], "--block-bootstrap expects"),
                         (["--tiles", 1000, "--block-bootstrap", 8, "--block-starts", 0], "--block-starts expects")):
        r = run_cli("-o", tmp, *graph, *extra, timeout=60)
        assert r.returncode == 2 and words in r.stderr, (extra, r.stderr)
    r = run_cli("-o", tmp, "--block-bootstrap", 8, timeout=60)                   # the window directories' mode
    assert r.returncode == 2 and "belongs to --regions FILE --pool and to --tiles SIZE" in r.stderr
    r = run_cli("-o", tmp, "--methylome", run["meth"], "--genome", "g", "--nodes", "n", "--edges", "e", "--block-bootstrap", 8,
                timeout=60)                                                       # the gene windows' mode
    assert r.returncode == 2 and "belongs to --regions FILE --pool and to --tiles SIZE" in r.stderr
    r = run_cli("--help", timeout=60)
    assert r.returncode == 0 and "--block-bootstrap R" in r.stdout and "block_raw.npy" in r.stdout
