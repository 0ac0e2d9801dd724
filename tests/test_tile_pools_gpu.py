"""Region pools on the device (abn_tiles_set_pools, alphabeta_rs_amd/csrc/abn_tiles.hpp: pools) against the mask model of
tests/_tile_pools_model.py: every pool's segments, source columns and pooled range, its per-sample rc_meth_lvl folds bit for
bit, its pairwise integers against the model and against the sums over its segments of what set_intervals gives; a pool
against a methylome cut down to the pool's lines; one interval per pool against the tiles of the same list; the switches
between pools and tiles (a refused tiles call and an empty interval list on a pooled handle among them); pools on handles
without a column and of one sample; the refusals; and `metaprofile_alphabeta --regions F --pool` against the directory path on a tree
whose k-th directory holds pool k's lines.

One refusal of abn_tiles_set_pools is not reached here: a pooled matrix beyond a handle's limits needs more than 256 x
INT32_MAX pooled columns, which over the 1 500 columns of these methylomes takes some 3.6e8 intervals (9 GB of arguments).
Its predicate, tiles_matrix_fits, is the one abn_tiles_create applies, and tests/test_tile_pools_cpu.py pins it at the limit."""
import ctypes as C
import struct

import numpy as np
import pytest

import _tile_pools_model as PM
import _tiles_model as T
import _windows_model as M
from _parse_model import HEADER
from test_tiles_gpu import (ALIGNS, FLT, INVALID, N, NAMES, NAN_SITE, L, bits, graph_files, handles, inputs, resident,  # noqa: F401
                            run_cli, tool_methylomes)

pytestmark = pytest.mark.gpu
RUN_ORDER = [2, 1, 257]


def model_of(rows, model, pools):
    """the model's answers for the pools over the aligned columns -> dict"""
    (ic, ilo, ihi, ip), names, _ = pools
    chrom, start, _, cols = model
    seg = PM.segments(RUN_ORDER, (ic, ilo, ihi), ip, len(names))
    cb, ce = T.search(chrom, start, (seg[1], seg[2], seg[3]))
    begin, end, src = PM.layout(PM.pool_columns(chrom, start, (ic, ilo, ihi), ip, len(names)))
    return {"segments": seg, "cb": cb, "ce": ce, "begin": begin, "end": end, "src": src, "cols": PM.pooled(cols, src)}


def everything(tiles):
    """every array a pooled handle gives, for byte comparisons"""
    return tiles.layout() + tiles.stats() + tiles.pairwise() + tiles.pool_segments() + (tiles.pool_columns(),)


def assert_same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()


@pytest.mark.parametrize("align", ALIGNS)
def test_pools_equal_the_model(abn, gpu_ctx, inputs, handles, align):
    rows, values, keeps = inputs
    h = handles[align]
    tiles, model = h["tiles"], h["model"]
    chrom, start, _, cols = model
    pools = PM.pool_list(rows)
    (ic, ilo, ihi, ip), names, _ = pools
    P = len(names)
    want = model_of(rows, model, pools)
    tiles.set_pools(ic, ilo, ihi, ip, P)
    assert tiles.info()["n_tiles"] == P and tiles.info()["n_columns"] == len(chrom)
    # the segments and their columns, the map, the pools' ranges
    seg = tiles.pool_segments()
    assert [a.dtype for a in seg] == [np.int32, np.int32, np.int64, np.int64, np.int64, np.int64]
    assert tuple(a.tolist() for a in seg[:4]) == tuple(want["segments"][:4])
    assert seg[4].tolist() == want["cb"].tolist() and seg[5].tolist() == want["ce"].tolist()
    src = tiles.pool_columns()
    assert src.dtype == np.int64 and src.tolist() == want["src"].tolist()
    begin, end = tiles.layout()
    assert begin.dtype == end.dtype == np.int64
    assert begin.tolist() == want["begin"].tolist() and end.tolist() == want["end"].tolist()
    # the folds: the host loop's bits, pool by pool
    count, lsk, kept = tiles.stats()
    want_sums, want_kept = T.folds(want["cols"], begin, end)
    assert count.tolist() == (end - begin).tolist() and kept.dtype == np.int64 and kept.tolist() == want_kept.tolist()
    want_bits = np.array([[struct.unpack("<Q", s)[0] for s in row] for row in want_sums], dtype=np.uint64).reshape(lsk.shape)
    assert np.array_equal(bits(lsk), want_bits)
    # the scan: the model's integers, and the sums over the pool's segments of what set_intervals gives (integers add exactly)
    diff, both, dval = tiles.pairwise()
    want_diff, want_both, want_dval = T.pairwise(want["cols"], begin, end)
    assert diff.dtype == both.dtype == np.uint64 and np.array_equal(diff, want_diff) and np.array_equal(both, want_both)
    assert np.array_equal(dval, want_dval, equal_nan=True) and np.array_equal(np.isnan(dval), both == 0)
    second = abn.Tiles.from_parsed(gpu_ctx, h["sites"], posterior_max_filter=FLT, align=align)
    try:
        second.set_intervals(seg[1], seg[2], seg[3])
        seg_diff, seg_both, _ = second.pairwise()
        sum_diff, sum_both = np.zeros_like(diff), np.zeros_like(both)
        np.add.at(sum_diff, seg[0], seg_diff)
        np.add.at(sum_both, seg[0], seg_both)
        assert np.array_equal(diff, sum_diff) and np.array_equal(both, sum_both)
        assert second.layout()[0].tolist() == seg[4].tolist() and second.layout()[1].tolist() == seg[5].tolist()
    finally:
        second.close()
    # a pool is no one interval
    with pytest.raises(abn.AbnError) as e:
        tiles.intervals()
    assert e.value.status == INVALID and "abn_tiles_pool_segments" in str(e.value)
    ms, pool_ms = tiles.kernel_ms(), tiles.pool_kernel_ms()
    assert ms.shape == (2,) and np.all(ms > 0) and pool_ms.shape == (4,) and np.all(pool_ms > 0)
    first = want["segments"][4]
    if align == "none":                                                        # the cases the pools are there for
        length = (seg[5] - seg[4]).tolist()
        assert {0, 1, 15, 16, 17, 63, 64, 65, 200} <= set(length)
        size = dict(zip(names, count.tolist()))
        assert size["nothing"] == 0 and size["one"] == 1 and size["lengths"] == 112 and size["wide"] == 329
        assert begin[names.index("wide")] % 64 != 0 and begin[names.index("one")] % 16 != 0 and len(src) > 256   # several workgroups
        a, b = src[begin[names.index("apart")]:end[names.index("apart")]].tolist()
        assert b - a == 300
        runs = src[begin[names.index("runs")]:end[names.index("runs")]]
        assert set(chrom[runs].tolist()) == {2, 1, 257} and np.all(np.diff(runs) > 0)          # run order 2, 1, C; each column once
        assert NAN_SITE in runs and start[runs[-1]] == T.LAST and {402, 403} <= set(runs.tolist())   # both strands at one start
        assert cols[1]["field"][NAN_SITE] < 3 and not cols[1]["counted"][NAN_SITE]
        assert {90 + 524 + k for k in range(20)} <= set(runs.tolist())                           # on both sides of the gap
        e = names.index("empties")                                             # thousands of empty segments in one wavefront
        assert first[e + 1] - first[e] == PM.N_EMPTY + 2 and size["empties"] == 2
    if align == "union":                                                       # placeholders: in the pool, and not counted
        at = names.index("shared")
        held = src[begin[at]:end[at]]
        placeholders = [int((c["code"][held] == 0x80).sum()) for c in cols]
        assert sum(placeholders) > 0
        assert kept[:, at].tolist() == [int(c["counted"][held].sum()) for c in cols]
        assert all(k + p <= len(held) for k, p in zip(kept[:, at].tolist(), placeholders))


def test_a_pool_equals_a_methylome_of_its_lines(abn, gpu_ctx, L, inputs, handles):
    """Codes.from_parsed on texts that hold one pool's lines: the existing, host-pinned fold and scan give the pool's stats
    and pairwise result bit for bit"""
    rows, values, keeps = inputs
    tiles = handles["none"]["tiles"]
    (ic, ilo, ihi, ip), names, _ = PM.pool_list(rows)
    tiles.set_pools(ic, ilo, ihi, ip, len(names))
    begin, end = tiles.layout()
    count, lsk, kept = tiles.stats()
    pairs = tiles.pairwise()
    src = tiles.pool_columns()
    for name in ("lengths", "wide", "apart", "runs", "shared", "empties"):
        p = names.index(name)
        keep = src[begin[p]:end[p]].tolist()                                   # align none: column k is line k
        sites = [resident(gpu_ctx, L, T.methylome_text(rows, values[s], keep=keep)) for s in range(N)]
        codes = abn.Codes.from_parsed(gpu_ctx, sites, posterior_max_filter=FLT)
        c, s, k = codes.stats()
        assert c.tolist() == [count[p]] * N and k.tolist() == kept[:, p].tolist(), name
        assert np.array_equal(bits(s), bits(lsk[:, p])), name
        for g, w in zip(pairs, codes.pairwise()):
            assert g[p].tobytes() == w.tobytes(), name
        codes.close()
        for x in sites:
            x.close()


@pytest.mark.parametrize("align", ALIGNS)
def test_one_interval_per_pool_equals_tiles(abn, gpu_ctx, inputs, handles, align):
    rows, values, keeps = inputs
    h = handles[align]
    explicit, _ = T.tile_list(rows)
    n = len(explicit[0])
    pooled = h["tiles"]
    pooled.set_pools(*explicit, np.arange(n), n)
    tiled = abn.Tiles.from_parsed(gpu_ctx, h["sites"], posterior_max_filter=FLT, align=align)
    try:
        tiled.set_intervals(*explicit)
        (pb, pe), (tb, te) = pooled.layout(), tiled.layout()
        assert (pe - pb).tobytes() == (te - tb).tobytes() and pb.tolist() == np.concatenate([[0], np.cumsum(te - tb)[:-1]]).tolist()
        assert_same(pooled.stats() + pooled.pairwise(), tiled.stats() + tiled.pairwise())
    finally:
        tiled.close()


def test_state_switches(abn, gpu_ctx, inputs, handles):
    rows, values, keeps = inputs
    h = handles["position"]
    (ic, ilo, ihi, ip), names, _ = PM.pool_list(rows)
    P = len(names)
    other = (ic[:9][::-1].copy(), ilo[:9][::-1].copy(), ihi[:9][::-1].copy(), np.array([2, 0, 0, 1, 2, 2, 0, 1, 1], dtype=np.int32))
    used = h["tiles"]
    fresh = abn.Tiles.from_parsed(gpu_ctx, h["sites"], posterior_max_filter=FLT, align="position")
    try:
        fresh.set_pools(ic, ilo, ihi, ip, P)
        used.set_pools(ic, ilo, ihi, ip, P)
        used.set_fixed(1 << 28)                                                # back on the handle's own matrix ...
        with pytest.raises(abn.AbnError):
            used.pool_segments()
        with pytest.raises(abn.AbnError):
            used.pool_columns()
        assert np.all(used.pool_kernel_ms() == 0)
        fresh.set_fixed(1 << 28)
        assert used.info() == fresh.info()
        assert_same(used.intervals() + used.layout() + used.stats() + used.pairwise(),
                    fresh.intervals() + fresh.layout() + fresh.stats() + fresh.pairwise())
        fresh.set_pools(ic, ilo, ihi, ip, P)
        used.set_pools(ic, ilo, ihi, ip, P)                                    # ... and on the pooled one again
        assert used.info() == fresh.info() and used.info()["n_tiles"] == P
        assert_same(everything(used), everything(fresh))
        used.set_pools(*other, 3)                                              # another list replaces the first
        again = abn.Tiles.from_parsed(gpu_ctx, h["sites"], posterior_max_filter=FLT, align="position")
        try:
            again.set_pools(*other, 3)
            assert used.info() == again.info() and used.info()["n_tiles"] == 3
            assert_same(everything(used), everything(again))
            assert used.layout()[1][-1] < fresh.layout()[1][-1]
        finally:
            again.close()
    finally:
        fresh.close()


def test_refusals(abn, gpu_ctx, inputs, handles):
    rows, values, keeps = inputs
    lib = gpu_ctx._L
    i32p, i64p = C.POINTER(C.c_int32), C.POINTER(C.c_int64)
    t = abn.Tiles.from_parsed(gpu_ctx, handles["none"]["sites"], posterior_max_filter=FLT)
    try:
        for getter in (t.pool_segments, t.pool_columns):                       # no pools yet
            with pytest.raises(abn.AbnError) as e:
                getter()
            assert e.value.status == INVALID and "abn_tiles_set_pools" in str(e.value)
        assert np.all(t.pool_kernel_ms() == 0)
        (ic, ilo, ihi, ip), names, _ = PM.pool_list(rows)
        t.set_pools(ic, ilo, ihi, ip, len(names))
        before = everything(t)

        def said():
            return (lib.abn_last_error(gpu_ctx._h) or b"").decode()

        one, c1, p1 = np.zeros(1, dtype=np.int64), np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.int32)
        p = lambda a, ty: a.ctypes.data_as(ty)
        full = [p(c1, i32p), p(one, i64p), p(one, i64p), p(c1, i32p)]
        # null / size
        assert lib.abn_tiles_set_pools(None, 0, None, None, None, None, 1) == INVALID
        assert lib.abn_tiles_set_pools(t._h, -1, *full, 1) == INVALID and "null/size" in said()
        for k in range(4):
            assert lib.abn_tiles_set_pools(t._h, 1, *[None if j == k else a for j, a in enumerate(full)], 1) == INVALID
            assert "null/size" in said()
        # the number of pools
        for n_pools, words in ((0, "n_pools"), (-3, "n_pools"), ((1 << 31), "INT32_MAX"), ((1 << 40), "INT32_MAX")):
            assert lib.abn_tiles_set_pools(t._h, 1, *full, n_pools) == INVALID and words in said(), n_pools
        # a pool id out of range: the text names the interval
        for ids, at in (([0, 3, 0], 1), ([0, 0, -1], 2), ([5, 0, 0], 0)):
            with pytest.raises(abn.AbnError) as e:
                t.set_pools([1, 1, 1], [0, 0, 0], [5, 5, 5], ids, 3)
            assert e.value.status == INVALID and f"interval {at}:" in str(e.value) and "pool" in str(e.value)
        # an interval tiles_interval_valid rejects
        for bad in (([258], [0], [5]), ([-1], [0], [5]), ([1], [-1], [5]), ([1], [0], [T.POS_END + 1]), ([1], [T.POS_END + 1], [5])):
            with pytest.raises(abn.AbnError) as e:
                t.set_pools(*bad, [0], 1)
            assert e.value.status == INVALID and "interval 0:" in str(e.value) and "2^32" in str(e.value)
        with pytest.raises(abn.AbnError) as e:
            t.set_pools([1, 1, 300], [0, 0, 0], [5, 5, 5], [0, 0, 0], 1)
        assert e.value.status == INVALID and "interval 2:" in str(e.value)
        with pytest.raises(ValueError):
            t.set_pools([1, 1], [0, 0], [5, 5], [0], 1)
        # a pooled handle's intervals
        with pytest.raises(abn.AbnError) as e:
            t.intervals()
        assert e.value.status == INVALID and "abn_tiles_pool_segments" in str(e.value)
        # behind every refusal the handle holds what it held, and takes the next list
        assert t.info()["n_tiles"] == len(names)
        assert_same(everything(t), before)
        t.set_pools([1], [T.POS_END], [0], [1], 2)                             # the bounds themselves are fine: two empty pools
        assert t.stats()[0].tolist() == [0, 0] and t.pool_segments()[0].shape == (0,) and t.pool_columns().shape == (0,)
        assert np.isnan(t.pairwise()[2]).all() and t.layout()[1].tolist() == [0, 0]
        t.set_pools([], [], [], [], 3)                                         # no interval: every pool is empty
        assert t.info()["n_tiles"] == 3 and t.stats()[2].tolist() == [[0, 0, 0]] * N
        for entry, args in ((lib.abn_tiles_pool_segments, (None,) * 7), (lib.abn_tiles_pool_columns, (None,)),
                            (lib.abn_tiles_pool_kernel_ms, (None,))):
            assert entry(None, *args) == INVALID
        assert lib.abn_tiles_pool_kernel_ms(t._h, None) == INVALID
    finally:
        t.close()


def test_a_refused_tiles_call_leaves_a_pooled_handle_as_it_was(abn, inputs, handles):
    rows, values, keeps = inputs
    t = handles["none"]["tiles"]
    (ic, ilo, ihi, ip), names, _ = PM.pool_list(rows)
    t.set_pools(ic, ilo, ihi, ip, len(names))
    info, before = t.info(), everything(t)
    refused = ((lambda: t.set_intervals([258], [0], [5]), "tile 0:"), (lambda: t.set_fixed(0), "tile size"),
               (lambda: t.set_fixed(1), "INT32_MAX"))                            # (a site at 4294967295: 2^32 tiles of one bp)
    for call, words in refused:
        with pytest.raises(abn.AbnError) as e:
            call()
        assert e.value.status == INVALID and words in str(e.value)
        assert t.info() == info and info["n_tiles"] == len(names)
        assert_same(everything(t), before)


def test_an_empty_interval_list_drops_the_pools(abn, gpu_ctx, inputs, handles):
    rows, values, keeps = inputs
    h = handles["position"]
    (ic, ilo, ihi, ip), names, _ = PM.pool_list(rows)
    used = h["tiles"]
    used.set_pools(ic, ilo, ihi, ip, len(names))
    used.set_intervals([], [], [])                                             # no tile, and the handle's own matrix again
    assert used.info()["n_tiles"] == 0
    for getter in (used.pool_segments, used.pool_columns):
        with pytest.raises(abn.AbnError) as e:
            getter()
        assert e.value.status == INVALID and "abn_tiles_set_pools" in str(e.value)
    assert np.all(used.pool_kernel_ms() == 0) and np.all(used.kernel_ms() == 0)
    fresh = abn.Tiles.from_parsed(gpu_ctx, h["sites"], posterior_max_filter=FLT, align="position")
    try:
        fresh.set_pools(ic, ilo, ihi, ip, len(names))
        used.set_pools(ic, ilo, ihi, ip, len(names))
        assert used.info() == fresh.info() and used.info()["n_tiles"] == len(names)
        assert_same(everything(used), everything(fresh))
    finally:
        fresh.close()


def test_pools_on_degenerate_handles(abn, gpu_ctx, L, inputs, handles):
    rows, values, keeps = inputs
    # two header-only methylomes: no column, no run — every pool is empty
    empties = [resident(gpu_ctx, L, HEADER.encode()) for _ in range(2)]
    none = abn.Tiles.from_parsed(gpu_ctx, empties, posterior_max_filter=FLT)
    try:
        assert none.info()["n_columns"] == 0 and none.n_runs == 0
        none.set_pools([1, 2], [0, 5], [T.POS_END, 9], [0, 1], 2)
        assert none.info()["n_tiles"] == 2 and none.layout()[0].tolist() == none.layout()[1].tolist() == [0, 0]
        count, lsk, kept = none.stats()
        assert count.tolist() == [0, 0] and kept.tolist() == [[0, 0]] * 2 and lsk.tolist() == [[0.0, 0.0]] * 2
        dval = none.pairwise()[2]
        assert dval.shape == (2, 1) and np.isnan(dval).all()
        assert all(a.shape == (0,) for a in none.pool_segments()) and none.pool_columns().shape == (0,)
    finally:
        none.close()
        for s in empties:
            s.close()
    # one sample: the stats work, the pairwise call writes nothing
    (ic, ilo, ihi, ip), names, _ = PM.pool_list(rows)
    n_pools = len(names)
    single = abn.Tiles.from_parsed(gpu_ctx, handles["none"]["sites"][:1], posterior_max_filter=FLT)
    try:
        single.set_pools(ic, ilo, ihi, ip, n_pools)
        count, lsk, kept = single.stats()
        assert count.shape == (n_pools,) and lsk.shape == kept.shape == (1, n_pools)
        want = handles["none"]["tiles"]
        want.set_pools(ic, ilo, ihi, ip, n_pools)
        assert count.tobytes() == want.stats()[0].tobytes() and kept[0].tobytes() == want.stats()[2][0].tobytes()
        filled = [np.full(n_pools, 7, dtype=np.uint64), np.full(n_pools, 7, dtype=np.uint64), np.full(n_pools, 7.0)]
        u64p = C.POINTER(C.c_uint64)
        assert gpu_ctx._L.abn_tiles_pairwise(single._h, filled[0].ctypes.data_as(u64p), filled[1].ctypes.data_as(u64p),
                                             filled[2].ctypes.data_as(C.POINTER(C.c_double))) == 0
        assert all((a == 7).all() for a in filled)
        assert all(a.shape == (n_pools, 0) for a in single.pairwise())
    finally:
        single.close()


# ---------------------------------------------------------------- the tool
TILE, PER_TILE = 1000, 100
POOLS = {"TE": [0, 9, 5], "gene": [1, 7, 2], "state_3": [3, 10]}             # the tiles of tool_methylomes a pool holds


def region_row(k, name=None):
    return f"chr1\t{TILE * k}\t{TILE * (k + 1)}" + (f"\t{name}\t0\t+" if name else "")


def test_metaprofile_pools_equal_the_directory_path(tmp_path):
    """three named pools of non-contiguous rows against the directory path on a tree whose k-th directory holds pool k's
    lines: raw.npy byte for byte, every results.txt column but `region`; pools.txt"""
    meth = tmp_path / "methylome"
    lines = tool_methylomes(meth)
    nodes, edges = graph_files(tmp_path, meth)
    names = list(POOLS)
    args = M.Args(step=100, size=100, absolute=False)                            # 3 regions x 1 window: 3 directories
    of = {name: sorted(POOLS[name]) for name in names}
    wins = {f: [[[{"original": l} for k in of[name] for l in lines[f][PER_TILE * k:PER_TILE * (k + 1)]]] for name in names] for f in NAMES}
    tree, out = tmp_path / "tree", tmp_path / "out"
    tree.mkdir(), out.mkdir()
    M.save_tree(tree, args, 100, nodes, edges, wins)
    (tmp_path / "dist.txt").write_text("".join(f"{PER_TILE * len(of[name])}\n" for name in names))
    common = ["--iterations", "20", "--seed", "77"]
    r1 = run_cli("-o", tree, "--distribution", tmp_path / "dist.txt", "-s", "100", "-w", "100", *common)
    assert r1.returncode == 0, r1.stdout[-2000:] + r1.stderr[-2000:]
    # the rows in no order, pools numbered by first appearance; a nested row, a row without a name, a header
    order = [("TE", 0), ("gene", 1), ("state_3", 3), ("TE", 9), ("gene", 7), (None, 4), ("TE", 5), ("gene", 2), ("state_3", 10)]
    rows = ["track name=classes"] + [region_row(k, name) for name, k in order] + ["chr1\t5200\t5800\tTE"]
    (tmp_path / "classes.bed").write_text("\n".join(rows) + "\n")
    graph = ["--methylome", meth, "--nodes", tmp_path / "nodelist.fn", "--edges", tmp_path / "edgelist.fn"]
    r2 = run_cli("-o", out, *graph, "--regions", tmp_path / "classes.bed", "--pool", *common)
    assert r2.returncode == 0, r2.stdout[-2000:] + r2.stderr[-2000:]
    want, got = (tree / "results.txt").read_text().splitlines(), (out / "results.txt").read_text().splitlines()
    assert len(want) == len(got) == 1 + len(names) and want[0] == got[0]
    assert (out / "raw.npy").read_bytes() == (tree / "raw.npy").read_bytes()
    assert np.load(out / "raw.npy").shape == (20, 7, len(names))
    for k, (w, g) in enumerate(zip(want[1:], got[1:])):
        w, g = w.split(";"), g.split(";")
        assert g[3] == names[k] and w[3] in M.REGIONS
        assert w[:3] + w[4:] == g[:3] + g[4:] and g[1] == str(k) and g[2] == str(PER_TILE * len(of[names[k]]))
    assert (out / "pools.txt").read_text() == ("pool;name;intervals;segments;cg_count;fitted\n"
                                               "0;TE;4;3;300;1\n1;gene;3;2;300;1\n2;state_3;2;2;200;1\n")   # (gene: two rows touch)
    assert not (out / "tiles.txt").exists()
    assert r2.stdout.count("Skipped 1 regions without a name") == 1 and "Error" not in r2.stdout


def test_metaprofile_pool_of_distinct_names_equals_regions(tmp_path):
    """every row its own name: the pools are the rows, and raw.npy has the bytes of the same list without --pool; an empty
    pool is reported and skipped as an empty tile is"""
    meth = tmp_path / "methylome"
    tool_methylomes(meth)
    graph_files(tmp_path, meth)
    rows = [region_row(k, f"bin{k}") for k in range(6)]
    rows.insert(2, "chr3\t0\t1000\tnowhere")
    (tmp_path / "bins.bed").write_text("\n".join(rows) + "\n")
    graph = ["--methylome", meth, "--nodes", tmp_path / "nodelist.fn", "--edges", tmp_path / "edgelist.fn"]
    common = ["--regions", tmp_path / "bins.bed", "--iterations", "20", "--seed", "77"]
    a, b = tmp_path / "a", tmp_path / "b"
    a.mkdir(), b.mkdir()
    r1, r2 = run_cli("-o", a, *graph, *common), run_cli("-o", b, *graph, *common, "--pool")
    assert r1.returncode == 0 and r2.returncode == 0, r1.stdout[-1500:] + r2.stdout[-1500:] + r2.stderr[-1500:]
    assert (a / "raw.npy").read_bytes() == (b / "raw.npy").read_bytes() and np.load(b / "raw.npy").shape == (20, 7, 6)
    ta, tb = ((d / "results.txt").read_text().splitlines() for d in (a, b))
    assert len(ta) == len(tb) == 7
    for x, y in zip(ta[1:], tb[1:]):
        x, y = x.split(";"), y.split(";")
        assert x[:3] + x[4:] == y[:3] + y[4:] and y[3].startswith("bin")
    listed = (b / "pools.txt").read_text().splitlines()
    assert listed[3] == "2;nowhere;1;0;0;0" and listed[4] == f"3;bin2;1;1;{PER_TILE};1" and len(listed) == 8
    assert r2.stdout.count("Error: Error while building pedigree: pool 2 (nowhere): no site lies in this pool") == 1
    assert r2.stdout.count("Error:") == 1 and (a / "tiles.txt").exists() and not (a / "pools.txt").exists()


def test_metaprofile_pool_flags_are_checked(tmp_path):
    graph = ["-o", tmp_path, "--methylome", tmp_path, "--nodes", "x", "--edges", "x"]
    (tmp_path / "bad.bed").write_text("chr1\t0\t1000\tTE\nchr1\t2000\t3000\tDNA;hAT\n")
    for extra, words in ((["--pool"], "--pool belongs to --regions"),
                         (["--tiles", "100", "--pool"], "--pool belongs to --regions"),
                         (["--regions", tmp_path / "bad.bed", "--pool"], "';'")):
        r = run_cli(*graph, *extra, timeout=60)
        assert r.returncode == 2 and words in r.stderr, (extra, r.stderr)
    r = run_cli("-o", tmp_path, "--pool", timeout=60)
    assert r.returncode == 2 and "--pool belongs to --regions" in r.stderr
    r = run_cli("--help", timeout=60)
    assert r.returncode == 0 and "--pool" in r.stdout and "pools.txt" in r.stdout
