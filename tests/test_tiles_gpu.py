"""Genomic tiles on the device (abn_tiles_*, alphabeta_rs_amd/csrc/abn_tiles.hpp) against the model of
tests/_tiles_model.py: every tile's column range, its per-sample rc_meth_lvl folds bit for bit, its pairwise result against
the scan of Codes.from_parsed's matrix over the same ranges; tiles against methylomes cut down to the tile's lines; the three
align modes; the refusals; and `metaprofile_alphabeta --tiles / --regions` against the directory path on a tree that holds
every tile's lines."""
import ctypes as C
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

import _parse_model as P
import _tiles_model as T
import _windows_model as M
from test_sites_resident_gpu import LONG, decide

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden"
FLT = T.FILTER
INVALID = 1  # ABN_ERR_INVALID_ARG
ALIGNS = ("none", "position", "union")
N = 4
NAN_SITE = 700          # of sample 1: its posterior is `nan`, a line the host decides


@pytest.fixture(scope="module")
def L():
    return P.hostlib()


def resident(ctx, L, text):
    """Context.parse_sites_resident as the pedigree build reads a file (every line), the host-decided lines inserted"""
    r = ctx.parse_sites_resident(text, skip_lines=0, slab_bytes=4096)
    r.insert(*decide(L, text, r.deferred()))
    return r


@pytest.fixture(scope="module")
def inputs():
    """the sites, every sample's values, and per align mode the sites every sample holds (none: all; else each lacks nine)"""
    rows = T.master_sites()
    values = [T.sample_values(rows, 40 + s, nan_at=NAN_SITE if s == 1 else None) for s in range(N)]
    rng = np.random.default_rng(5)
    lacking = [sorted(set(range(len(rows))) - set(rng.choice(NAN_SITE - 1, size=9, replace=False).tolist())) for _ in range(N)]
    keeps = {"none": [list(range(len(rows)))] * N, "position": lacking, "union": lacking}
    return rows, values, keeps


@pytest.fixture(scope="module")
def handles(abn, gpu_ctx, L, inputs):
    """per align mode: the resident sites, the Tiles and the Codes made of them, and the model's columns"""
    rows, values, keeps = inputs
    made = {}
    for align in ALIGNS:
        sites = [resident(gpu_ctx, L, T.methylome_text(rows, values[s], keeps[align][s])) for s in range(N)]
        made[align] = {"sites": sites, "tiles": abn.Tiles.from_parsed(gpu_ctx, sites, posterior_max_filter=FLT, align=align),
                       "codes": abn.Codes.from_parsed(gpu_ctx, sites, posterior_max_filter=FLT, align=align),
                       "model": T.aligned(rows, values, keeps[align], align)}
    yield made
    for m in made.values():
        m["tiles"].close(), m["codes"].close()
        for s in m["sites"]:
            s.close()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def assert_tiles_equal_model(gpu_ctx, tiles, codes, model, want_intervals):
    """layout, stats and pairwise of the handle's current tiles against the model and the scan of the Codes matrix"""
    chrom, start, _, cols = model
    got_iv = tiles.intervals()
    assert [a.dtype for a in got_iv] == [np.int32, np.int64, np.int64]
    assert all(g.tolist() == np.asarray(w).tolist() for g, w in zip(got_iv, want_intervals))
    begin, end = tiles.layout()
    want_b, want_e = T.search(chrom, start, want_intervals)
    assert begin.dtype == end.dtype == np.int64
    assert begin.tolist() == want_b.tolist() and end.tolist() == want_e.tolist()
    count, lsk, kept = tiles.stats()
    want_sums, want_kept = T.folds(cols, begin, end)
    assert count.tolist() == (want_e - want_b).tolist() and kept.dtype == np.int64 and kept.tolist() == want_kept.tolist()
    want_bits = np.array([[struct.unpack("<Q", s)[0] for s in row] for row in want_sums], dtype=np.uint64).reshape(lsk.shape)
    assert np.array_equal(bits(lsk), want_bits)                                  # the host loop's bits, tile by tile
    got = tiles.pairwise()
    want = gpu_ctx.pairwise_divergence_windows_packed(codes.packed(), codes.n_sites, begin, end)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes()   # dvalue: NaN in the same places
    diff, both, dval = T.pairwise(cols, begin, end)
    assert np.array_equal(got[0], diff) and np.array_equal(got[1], both)
    assert np.array_equal(got[2], dval, equal_nan=True) and np.isnan(got[2][both == 0]).all()
    return begin, end, kept


@pytest.mark.parametrize("align", ALIGNS)
def test_tiles_equal_the_model_and_the_codes_scan(abn, gpu_ctx, inputs, handles, align):
    rows, values, keeps = inputs
    h = handles[align]
    tiles, codes, model = h["tiles"], h["codes"], h["model"]
    chrom, start, _, cols = model
    runs = T.runs_of(chrom, start)
    assert tiles.info() == {"n_samples": N, "n_columns": len(chrom), "row_stride": codes.row_stride, "n_runs": 3,
                            "n_tiles": tiles.info()["n_tiles"]}
    assert codes.n_sites == len(chrom)
    got_runs = tiles.runs()
    assert [a.dtype for a in got_runs] == [np.int32, np.int64, np.int64, np.uint32]
    assert list(zip(*(a.tolist() for a in got_runs))) == runs and [r[0] for r in runs] == [2, 1, 257]   # run order, not key order
    explicit, names = T.tile_list(rows)
    tiles.set_intervals(*explicit)
    begin, end, kept = assert_tiles_equal_model(gpu_ctx, tiles, codes, model, explicit)
    ms = tiles.kernel_ms()
    assert ms.shape == (2,) and np.all(ms > 0)
    length = (end - begin).tolist()
    if align == "none":
        assert {0, 1, 63, 64, 65, 200} <= set(length) and 0 in begin.tolist()
        assert (begin % 16 != 0).any() and (begin % 64 != 0).any()
        assert end[names.index("run's last column")] == runs[0][2] and begin[names.index("C from 0")] == runs[2][1]
        assert length[names.index("both strands")] == 2 and length[names.index("up to 2^32")] == 1
        assert length[names.index("over the gap")] == 20 and length[names.index("no such chromosome")] == 0
        at = names.index("whole run 1")                                          # holds the NaN posterior of sample 1
        assert cols[1]["field"][NAN_SITE] < 3 and not cols[1]["counted"][NAN_SITE] and begin[at] <= NAN_SITE < end[at]
    for size, step in ((1 << 28, 0), (1 << 30, 1 << 29)):                        # step < size: overlapping tiles
        tiles.set_fixed(size, step)
        fixed = T.fixed_intervals(runs, size, step)
        begin, end, kept = assert_tiles_equal_model(gpu_ctx, tiles, codes, model, fixed)
        assert len(begin) == sum(-(-(r[3] + 1) // (step or size)) for r in runs)
    if align == "union":                                                         # a placeholder is not counted
        whole = (np.array([r[0] for r in runs], dtype=np.int32), np.zeros(3, dtype=np.int64), np.full(3, T.POS_END, dtype=np.int64))
        tiles.set_intervals(*whole)
        count, lsk, kept = tiles.stats()
        own = abn.Codes.from_parsed(gpu_ctx, h["sites"], posterior_max_filter=FLT)     # unaligned: every sample's own sites
        assert kept.sum(axis=1).tolist() == own.stats()[2].tolist() and count.sum() == len(chrom)
        assert (own.stats()[0] < len(chrom)).all()
        own.close()


def test_a_tile_equals_a_methylome_of_its_lines(abn, gpu_ctx, L, inputs, handles):
    """Codes.from_parsed on texts that hold one tile's lines: the existing, host-pinned fold and scan give the tile's stats
    and pairwise result bit for bit"""
    rows, values, keeps = inputs
    tiles = handles["none"]["tiles"]
    explicit, names = T.tile_list(rows)
    tiles.set_intervals(*explicit)
    begin, end = tiles.layout()
    count, lsk, kept = tiles.stats()
    pairs = tiles.pairwise()
    for name in ("65 columns", "200 columns", "whole run 1", "both strands"):
        t = names.index(name)
        sites = [resident(gpu_ctx, L, T.methylome_text(rows, values[s], range(begin[t], end[t]))) for s in range(N)]
        codes = abn.Codes.from_parsed(gpu_ctx, sites, posterior_max_filter=FLT)
        c, s, k = codes.stats()
        assert c.tolist() == [count[t]] * N and k.tolist() == kept[:, t].tolist(), name
        assert np.array_equal(bits(s), bits(lsk[:, t])), name
        for g, w in zip(pairs, codes.pairwise()):
            assert g[t].tobytes() == w.tobytes(), name
        codes.close()
        for x in sites:
            x.close()


def test_set_intervals_again_equals_a_fresh_handle(abn, gpu_ctx, inputs, handles):
    rows, values, keeps = inputs
    h = handles["position"]
    explicit, _ = T.tile_list(rows)
    second = (explicit[0][::-1][:7].copy(), explicit[1][::-1][:7].copy(), explicit[2][::-1][:7].copy())
    used = h["tiles"]
    used.set_intervals(*explicit)
    first_layout = used.layout()
    used.set_intervals(*second)
    fresh = abn.Tiles.from_parsed(gpu_ctx, h["sites"], posterior_max_filter=FLT, align="position")
    fresh.set_intervals(*second)
    try:
        assert used.info() == fresh.info() and used.info()["n_tiles"] == 7 and len(first_layout[0]) == len(explicit[0])
        for a, b in zip(used.intervals() + used.layout() + used.stats() + used.pairwise(),
                        fresh.intervals() + fresh.layout() + fresh.stats() + fresh.pairwise()):
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
        used.set_intervals([], [], [])                                           # no tile: an empty list, not an error
        assert used.info()["n_tiles"] == 0 and used.stats()[1].shape == (N, 0) and used.pairwise()[0].shape == (0, N * (N - 1) // 2)
    finally:
        fresh.close()


def test_refusals(abn, gpu_ctx, L, inputs, handles):
    rows, values, keeps = inputs
    lib = gpu_ctx._L
    i32p, i64p = C.POINTER(C.c_int32), C.POINTER(C.c_int64)
    # align none: every sample must have sample 0's number of sites, and the text names --align
    lacking = handles["position"]["sites"]
    shorter = resident(gpu_ctx, L, T.methylome_text(rows, values[0], range(50)))
    with pytest.raises(abn.AbnError) as e:
        abn.Tiles.from_parsed(gpu_ctx, [lacking[0], shorter], posterior_max_filter=FLT)
    assert e.value.status == INVALID and "--align" in str(e.value)
    # ... and sample 0 must be well ordered: the refusals of the common-site step
    texts = {"split run": [0, 1, 600, 2], "not ascending": [0, 2, 1], "not ascending ": [300, 301, 301]}
    for words, order in texts.items():
        bad = resident(gpu_ctx, L, T.methylome_text(rows, values[0], order))
        with pytest.raises(abn.AbnError) as e:
            abn.Tiles.from_parsed(gpu_ctx, [bad, bad], posterior_max_filter=FLT)
        assert e.value.status == INVALID and words.strip() in str(e.value), str(e.value)
        bad.close()
    shorter.close()
    # the getters of tiles before any set_*
    t = abn.Tiles.from_parsed(gpu_ctx, handles["none"]["sites"], posterior_max_filter=FLT)
    assert t.info()["n_tiles"] == -1
    for getter in (t.intervals, t.layout, t.stats, t.pairwise):
        with pytest.raises(abn.AbnError) as e:
            getter()
        assert e.value.status == INVALID
    assert np.all(t.kernel_ms() == 0) and len(t.runs()[0]) == 3
    # bad intervals
    for bad in (([258], [0], [5]), ([-1], [0], [5]), ([1], [-1], [5]), ([1], [0], [T.POS_END + 1]), ([1], [T.POS_END + 1], [5]),
                ([1, 1, 300], [0, 0, 0], [5, 5, 5])):
        with pytest.raises(abn.AbnError) as e:
            t.set_intervals(*bad)
        assert e.value.status == INVALID
    assert t.info()["n_tiles"] == -1
    one = np.zeros(1, dtype=np.int64)
    c1 = np.zeros(1, dtype=np.int32)
    p = lambda a, ty: a.ctypes.data_as(ty)
    assert lib.abn_tiles_set_intervals(t._h, -1, p(c1, i32p), p(one, i64p), p(one, i64p)) == INVALID
    assert lib.abn_tiles_set_intervals(t._h, 1, None, p(one, i64p), p(one, i64p)) == INVALID
    assert lib.abn_tiles_set_intervals(t._h, 1, p(c1, i32p), None, p(one, i64p)) == INVALID
    assert lib.abn_tiles_set_intervals(t._h, 1, p(c1, i32p), p(one, i64p), None) == INVALID
    assert lib.abn_tiles_set_intervals(None, 0, None, None, None) == INVALID
    for size, step in ((0, 0), (-3, 0), (5, -1)):
        with pytest.raises(abn.AbnError) as e:
            t.set_fixed(size, step)
        assert e.value.status == INVALID
    with pytest.raises(abn.AbnError) as e:                                      # a site at 4294967295: 2^32 tiles of one bp
        t.set_fixed(1)
    assert e.value.status == INVALID and "INT32_MAX" in str(e.value)
    t.set_intervals([1], [T.POS_END], [0])                                       # the bounds themselves are fine
    assert t.layout()[0].tolist() == t.layout()[1].tolist()
    t.close()
    # abn_tiles_create refuses what abn_codes_create_* refuse
    def create(handles_, ctx=gpu_ctx, n=None, align=0, out=True):
        raw = [h._h if hasattr(h, "_h") else h for h in handles_]
        arr = (C.c_void_p * max(len(raw), 1))(*(h.value if isinstance(h, C.c_void_p) else h for h in raw))
        w = C.c_void_p(0xdead)
        rc = lib.abn_tiles_create(ctx._h if ctx else None, FLT, align, len(raw) if n is None else n, arr, C.byref(w) if out else None)
        if rc and ctx and out:
            assert not w.value
        return rc

    good = handles["none"]["sites"][0]
    text = (P.HEADER + "\n".join([P.cg_line(pos="5"), P.cg_line(pos="6", pm=LONG), P.cg_line(pos="7")]) + "\n").encode()
    r = gpu_ctx.parse_sites_resident(text, skip_lines=0)
    assert r.info()["n_deferred"] == 1 and create([r]) == INVALID                # the forgotten insert
    r.close()
    assert create([good], ctx=None) == INVALID and create([good], out=False) == INVALID
    assert create([], n=0) == INVALID and create([good], n=-1) == INVALID and create([good, None]) == INVALID
    assert create([good], align=3) == INVALID and create([good], align=-1) == INVALID
    host = C.c_void_p()
    assert lib.abn_sites_parse(gpu_ctx._h, text, len(text), None, C.byref(host)) == 0
    assert create([host]) == INVALID                                            # a host-form handle
    lib.abn_sites_destroy(host)
    other = abn.Context(0)
    try:
        foreign = other.parse_sites_resident(P.plain_text(20, seed=1), skip_lines=0)
        assert create([foreign]) == INVALID and create([good], ctx=other) == INVALID   # a sites handle of another context
        foreign.close()
    finally:
        other.close()
    for entry, n_args in ((lib.abn_tiles_destroy, 0), (lib.abn_tiles_info, 5), (lib.abn_tiles_runs, 4), (lib.abn_tiles_set_fixed, 2),
                          (lib.abn_tiles_intervals, 3), (lib.abn_tiles_layout, 2), (lib.abn_tiles_stats, 3),
                          (lib.abn_tiles_pairwise, 3), (lib.abn_tiles_kernel_ms, 1)):
        args = (5, 0) if entry is lib.abn_tiles_set_fixed else (None,) * n_args
        assert entry(None, *args) == INVALID
    # fewer than two samples: the stats work, the pairwise call writes nothing
    single = abn.Tiles.from_parsed(gpu_ctx, [good], posterior_max_filter=FLT)
    single.set_intervals([2], [0], [T.POS_END])
    count, lsk, kept = single.stats()
    assert count.tolist() == [524] and kept.shape == (1, 1) and 0 < kept[0, 0] < 524
    d = np.full(1, 7, dtype=np.uint64)
    assert lib.abn_tiles_pairwise(single._h, d.ctypes.data_as(C.POINTER(C.c_uint64)), None, None) == 0 and d[0] == 7
    single.close()
    # no site at all: no run, every tile empty
    empties = [resident(gpu_ctx, L, P.HEADER.encode()) for _ in range(2)]
    none = abn.Tiles.from_parsed(gpu_ctx, empties, posterior_max_filter=FLT)
    none.set_intervals([1, 2], [0, 5], [T.POS_END, 9])
    assert none.info()["n_columns"] == 0 and none.n_runs == 0 and none.stats()[0].tolist() == [0, 0]
    assert np.isnan(none.pairwise()[2]).all()
    none.set_fixed(100)
    assert none.info()["n_tiles"] == 0
    none.close()
    for s in empties:
        s.close()


def test_create_refuses_what_the_codes_entry_refuses(abn, gpu_ctx, L):
    """abn_tiles_create and Tiles.from_parsed on methylomes of three lines: a null handle in the list, a host-form handle, a
    handle of a second context and a handle with a deferred line and no insert are ABN_ERR_INVALID_ARG with the very text
    abn_codes_create_parsed gives; so are n_samples == 0 and an align outside 0..2 (which from_parsed refuses before the
    entry: its align names no such mode)"""
    lib = gpu_ctx._L
    text = (P.HEADER + "\n".join(P.cg_line(pos=str(p)) for p in (5, 6, 7)) + "\n").encode()
    deferring = (P.HEADER + "\n".join([P.cg_line(pos="5"), P.cg_line(pos="6", pm=LONG), P.cg_line(pos="7")]) + "\n").encode()

    class Raw:                                                                    # what from_parsed reads of a Sites
        def __init__(self, h):
            self._h = h

    def last_error(ctx):
        return (lib.abn_last_error(ctx._h) or b"").decode()

    def refused(samples, ctx=gpu_ctx, align=0):
        """the raw entry's status and text, the codes entry's, and from_parsed's -> the text"""
        arr = (C.c_void_p * max(len(samples), 1))(*(s._h.value if isinstance(s._h, C.c_void_p) else s._h for s in samples))
        w = C.c_void_p(0xdead)
        assert lib.abn_tiles_create(ctx._h, FLT, align, len(samples), arr, C.byref(w)) == INVALID and not w.value
        said = last_error(ctx)
        if 0 <= align <= 2:
            w = C.c_void_p(0xdead)
            assert lib.abn_codes_create_parsed(ctx._h, FLT, len(samples), arr, C.byref(w)) == INVALID and not w.value
            assert said == last_error(ctx) and said
            with pytest.raises(abn.AbnError) as e:
                abn.Tiles.from_parsed(ctx, samples, posterior_max_filter=FLT, align=("none", "position", "union")[align])
            assert e.value.status == INVALID and str(e.value).endswith(": " + said)
        return said

    good = resident(gpu_ctx, L, text)
    other = abn.Context(0)
    host = C.c_void_p()
    try:
        assert lib.abn_sites_parse(gpu_ctx._h, text, len(text), None, C.byref(host)) == 0
        foreign = other.parse_sites_resident(text, skip_lines=0)
        forgotten = gpu_ctx.parse_sites_resident(deferring, skip_lines=0)
        assert forgotten.info()["n_deferred"] == 1
        fine = abn.Tiles.from_parsed(gpu_ctx, [good, good], posterior_max_filter=FLT)   # the good handle is one
        assert fine.info()["n_columns"] == 3
        fine.close()
        texts = [refused([good, bad], align=align) for align in (0, 1, 2)
                 for bad in (Raw(None), Raw(host), foreign, forgotten)]
        assert texts[:4] == texts[4:8] == texts[8:] and len(set(texts[:4])) == 4
        assert [t for t in texts[:4]] == ["a null sites handle", "a sites handle in the host form (abn_sites_parse)",
                                          "a sites handle of another context",
                                          "a sites handle with deferred lines and no abn_sites_insert"]
        assert refused([good], ctx=other) == texts[2]                                # ... and the context's own side of it
        refused([])                                                                  # n_samples == 0
        refused([good], align=3), refused([good], align=-1)
        for align in (3, -1, "both"):
            with pytest.raises(ValueError):
                abn.Tiles.from_parsed(gpu_ctx, [good], posterior_max_filter=FLT, align=align)
        foreign.close(), forgotten.close()
    finally:
        if host.value:
            lib.abn_sites_destroy(host)
        other.close()
        good.close()


# ---------------------------------------------------------------- the tool
NAMES =["G0.txt", "G1_2.txt", "G4_2.txt", "G4_8.txt"]
TILE, PER_TILE, N_TILES = 1000, 100, 12


def tool_methylomes(meth: Path):
    """four methylomes of the bundled pedigree's sampled nodes: 1200 sites on chromosome 1, 100 in every 1000 bp, the later
    generations' statuses drifting from the founder's -> {name: [site line, ..]}"""
    rng = np.random.default_rng(8)
    n = PER_TILE * N_TILES
    status = rng.choice([0, 2], size=n, p=[0.6, 0.4])
    lines = {}
    meth.mkdir()
    for k, name in enumerate(NAMES):
        if k:
            status = np.where(rng.random(n) < 0.04 * k, rng.integers(0, 3, size=n), status)
        lines[name] = [M.site_line("1", 10 * i + 5, "+-"[i % 2], "UIM"[int(s)], [0.9999, 0.7][int(rng.integers(10) == 0)],
                                   round(float(0.05 + 0.45 * s + 0.04 * rng.random()), 4)) for i, s in enumerate(status)]
        (meth / name).write_text(M.HEADER + "".join(l + "\n" for l in lines[name]))
    return lines


def graph_files(tmp_path: Path, meth: Path):
    nodes = "filename\tnode\tgen\tmeth\n" + "".join(
        f"{meth}/{f}\t{node}\t{gen}\t{m}\n" for f, node, gen, m in
        [("G0.txt", "0_0", 0, "Y"), ("G1_2.txt", "1_2", 1, "Y"), ("G1_8.txt", "1_8", 1, "N"), ("G2_2.txt", "2_2", 2, "N"),
         ("G2_8.txt", "2_8", 2, "N")]) + "-\t3_2\t3\tN\n-\t3_8\t3\tN\n" + f"{meth}/G4_2.txt\t4_2\t4\tY\n{meth}/G4_8.txt\t4_8\t4\tY\n"
    edges = (GOLDEN / "data" / "edgelist.txt").read_text()
    (tmp_path / "nodelist.fn").write_text(nodes)
    (tmp_path / "edgelist.fn").write_text(edges)
    return nodes, edges


def run_cli(*args, timeout=300):
    from alphabeta_rs_amd import build as B

    B.build_host()
    return subprocess.run([str(B.META_CLI), *map(str, args)], capture_output=True, text=True, timeout=timeout)


def test_metaprofile_tiles_equal_the_directory_path(tmp_path):
    """12 fixed tiles against the existing directory path on a tree whose k-th (region, window) directory holds tile k's
    lines: raw.npy byte for byte, every results.txt column but `region`"""
    meth = tmp_path / "methylome"
    lines = tool_methylomes(meth)
    nodes, edges = graph_files(tmp_path, meth)
    args = M.Args(step=25, size=25, absolute=False)                              # 3 regions x 4 windows: 12 directories
    wins = {name: [[[{"original": l} for l in lines[name][PER_TILE * (4 * r + w):PER_TILE * (4 * r + w + 1)]] for w in range(4)]
                   for r in range(3)] for name in NAMES}
    tree, out = tmp_path / "tree", tmp_path / "out"
    tree.mkdir(), out.mkdir()
    M.save_tree(tree, args, 100, nodes, edges, wins)
    (tmp_path / "dist.txt").write_text(f"{PER_TILE}\n" * N_TILES)
    common = ["--iterations", "20", "--seed", "77"]
    r1 = run_cli("-o", tree, "--distribution", tmp_path / "dist.txt", "-s", "25", "-w", "25", *common)
    assert r1.returncode == 0, r1.stdout[-2000:] + r1.stderr[-2000:]
    graph = ["--methylome", meth, "--nodes", tmp_path / "nodelist.fn", "--edges", tmp_path / "edgelist.fn"]
    r2 = run_cli("-o", out, *graph, "--tiles", TILE, *common)
    assert r2.returncode == 0, r2.stdout[-2000:] + r2.stderr[-2000:]
    want, got = (tree / "results.txt").read_text().splitlines(), (out / "results.txt").read_text().splitlines()
    assert len(want) == len(got) == 1 + N_TILES and want[0] == got[0]            # neither side hides a failed tile
    assert (out / "raw.npy").read_bytes() == (tree / "raw.npy").read_bytes()
    assert np.load(out / "raw.npy").shape == (20, 7, N_TILES)
    for k, (w, g) in enumerate(zip(want[1:], got[1:])):
        w, g = w.split(";"), g.split(";")
        assert g[3] == f"1:{TILE * k}-{TILE * (k + 1)}" and w[3] in M.REGIONS
        assert w[:3] + w[4:] == g[:3] + g[4:] and g[1] == str(k) and g[2] == str(PER_TILE)
    assert (out / "tiles.txt").read_text() == "tile;chromosome;start;end;cg_count;fitted\n" + "".join(
        f"{k};1;{TILE * k};{TILE * (k + 1)};{PER_TILE};1\n" for k in range(N_TILES))
    assert "Error" not in r2.stdout and "Aligned by" not in r2.stdout
    # the same tiles as a region list with one empty region among them: exactly that tile is skipped; --align union says so
    regions = [f"chr1\t{TILE * k}\t{TILE * (k + 1)}\tbin{k}" for k in range(N_TILES)]
    regions.insert(5, "chr3 0 1000")
    (tmp_path / "regions.bed").write_text("track name=bins\n" + "\n".join(regions) + "\n")
    out2 = tmp_path / "out2"
    out2.mkdir()
    r3 = run_cli("-o", out2, *graph, "--regions", tmp_path / "regions.bed", "--align", "union", *common)
    assert r3.returncode == 0, r3.stdout[-2000:] + r3.stderr[-2000:]
    got = (out2 / "results.txt").read_text().splitlines()[1:]
    assert [int(l.split(";")[1]) for l in got] == [k for k in range(N_TILES + 1) if k != 5]
    assert np.load(out2 / "raw.npy").shape == (20, 7, N_TILES)
    listed = (out2 / "tiles.txt").read_text().splitlines()
    assert listed[0] == "tile;chromosome;start;end;cg_count;fitted" and len(listed) == N_TILES + 2
    assert [l.split(";")[5] for l in listed[1:]] == ["0" if k == 5 else "1" for k in range(N_TILES + 1)]
    assert listed[6] == "5;3;0;1000;0;0" and listed[7] == f"6;1;{5 * TILE};{6 * TILE};{PER_TILE};1"
    assert r3.stdout.count("Error: Error while building pedigree: tile 5 (3:0-1000):") == 1 and r3.stdout.count("Error:") == 1
    assert r3.stdout.count("Aligned by union: ") == 4 and f"G0.txt: {PER_TILE * N_TILES} sites, {PER_TILE * N_TILES} in the union" in r3.stdout
    for w, g in zip(want[1:6], got[:5]):                                         # the tiles in front of it: the same fits
        assert w.split(";")[4:] == g.split(";")[4:]


def test_metaprofile_tile_flags_are_checked(tmp_path):
    graph = ["-o", tmp_path, "--methylome", tmp_path, "--nodes", "x", "--edges", "x"]
    for extra, words in ((["--tiles", "100", "--regions", "r.bed"], "exclude each other"),
                         (["--tiles", "100", "--genome", "g.txt"], "--genome"),
                         (["--tiles", "100", "-a"], "-a"),
                         (["--tiles", "100", "--cutoff-gene-length"], "--cutoff-gene-length"),
                         (["--regions", "r.bed", "--invert"], "--invert"),
                         (["--tiles", "100", "--parse", "host"], "--parse host"),
                         (["--regions", "r.bed", "--sites", "host"], "--sites host"),
                         (["--tile-step", "50"], "--tile-step belongs to --tiles"),
                         (["--tiles", "0"], "--tiles expects"), (["--tiles", "1e3"], "--tiles expects"),
                         (["--tiles", "100", "--tile-step", "-5"], "--tile-step expects")):
        r = run_cli(*graph, *extra, timeout=60)
        assert r.returncode == 2 and words in r.stderr, (extra, r.stderr)
    r = run_cli("-o", tmp_path, "--tiles", "100", timeout=60)
    assert r.returncode == 2 and "need --methylome, --nodes and --edges" in r.stderr
    r = run_cli("--help", timeout=60)
    assert r.returncode == 0 and "--tiles SIZE" in r.stdout and "--regions FILE" in r.stdout and "tiles.txt" in r.stdout
