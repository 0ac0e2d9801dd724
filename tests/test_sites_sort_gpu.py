"""The sort of resident methylomes by genomic position on the device (abn_sites_sort, abn_sites_sort_keys): the primitive
on raw key arrays and the sorted handle against numpy.lexsort — stable, and never the code under test — exactly; the
builders on the sorted handles of shuffled files against the same builders on the files put in canonical order by the
Python model, byte for byte; and the tools' --sort."""
import ctypes as C
from functools import lru_cache
from pathlib import Path

import numpy as np
import pytest

import _parse_model as P
import _sort_model as M
import test_sites_split_gpu as S   # its texts and helpers, as they are

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden"
FLT = 0.99
KEYS = [k for k in S.KEYS if k != "line"]
SHUFFLED_TEXTS = tuple((name, M.shuffled_text(text, seed=41 + i)) for i, (name, text) in enumerate(S.SPLIT_TEXTS))


@pytest.fixture(scope="module")
def L():
    return M.hostlib()


# ---------------------------------------------------------------- the primitive
@lru_cache(maxsize=None)
def cases():
    """(n, pattern name, keys) of every primitive case, made once"""
    out = []
    for n in M.sizes(M.hostlib()):
        for name, k in M.patterns(n, seed=n):
            for a in k:
                a.setflags(write=False)
            out.append((n, name, k))
    return tuple(out)


def test_primitive_sizes_are_the_tile_edges(L):
    t = M.tile(L)
    assert t == 2048 and M.sizes(L) == (0, 1, 2, 63, 64, 65, t - 1, t, t + 1, 3 * t + 17)
    assert {name for _, name, _ in cases()} == {"three values", "full ranges", "all equal", "sorted", "reversed", "extremes",
                                                "by strand"}


@pytest.mark.parametrize("pattern", ["three values", "full ranges", "all equal", "sorted", "reversed", "extremes", "by strand"])
def test_primitive_equals_lexsort(gpu_ctx, pattern):
    for n, name, k in cases():
        if name != pattern:
            continue
        want, descents, equal = M.reference(k)
        order, info = gpu_ctx.sort_sites(*k)
        assert np.array_equal(order, want), (n, name)
        assert info == {"sites": n, "descents": descents, "equal": equal, "passes": M.passes_needed(k, descents)}, (n, name)
        if name in ("all equal", "sorted"):
            assert np.array_equal(order, np.arange(n)) and info["descents"] == 0 and info["passes"] == 0
        if name == "extremes" and n > 64:
            assert {0, 255, 256, 257} == set(k[0].tolist()) and {0, 0xffffffff} == set(k[1].tolist())


def test_primitive_sorts_by_every_key_bit(gpu_ctx):
    pairs = M.bit_pairs()
    assert [b for b, _ in pairs] == list(range(M.KEY_BITS))
    for bit, k in pairs:
        order, info = gpu_ctx.sort_sites(*k)
        assert order.tolist() == [1, 0] and (info["descents"], info["equal"], info["passes"]) == (1, 0, 1), bit


def test_primitive_refusals(abn, gpu_ctx):
    lib = gpu_ctx._L
    for bad in ((258, 0, 0, 0), (-1, 0, 0, 0), (0, 0, 0, 3)):
        with pytest.raises(abn.AbnError) as e:
            gpu_ctx.sort_sites(*([0, v] for v in bad))
        assert e.value.status == 1
    info = np.zeros(4, dtype=np.int64)
    i64p = C.POINTER(C.c_int64)
    assert lib.abn_sites_sort_keys(gpu_ctx._h, 1, None, None, None, None, None, info.ctypes.data_as(i64p)) == 1
    assert lib.abn_sites_sort_keys(gpu_ctx._h, 0, None, None, None, None, None, None) == 1
    assert lib.abn_sites_sort_keys(gpu_ctx._h, 1 << 32, None, None, None, None, None, info.ctypes.data_as(i64p)) == 1
    assert lib.abn_sites_sort_keys(None, 0, None, None, None, None, None, info.ctypes.data_as(i64p)) == 1
    assert lib.abn_sites_sort_keys_dev(gpu_ctx._h, 1, None, None, None, None, None, info.ctypes.data_as(i64p), None) == 1
    assert lib.abn_sites_sort_keys_dev(gpu_ctx._h, 0, None, None, None, None, None, info.ctypes.data_as(i64p), None) == 0


def test_primitive_on_device_arrays(gpu_ctx):
    """Keys and order stay in HBM.  The device buffers come from the HIP runtime the product library already holds, as in
    tests/test_pairwise_windows.py::test_windows_device_resident_entry."""
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipFree.argtypes = [C.c_void_p]
    lib = gpu_ctx._L
    n, name, k = next(c for c in cases() if c[0] == 3 * 2048 + 17 and c[1] == "three values")
    bufs = [C.c_void_p() for _ in range(5)]
    for ptr, size in zip(bufs, (4 * n, 4 * n, 4 * n, n, 4 * n)):
        assert hip.hipMalloc(C.byref(ptr), size) == 0
    try:
        for ptr, a in zip(bufs, k):
            assert hip.hipMemcpy(ptr, a.ctypes.data, a.nbytes, 1) == 0
        info, ms, order = np.zeros(4, dtype=np.int64), np.zeros(2), np.zeros(n, dtype=np.uint32)
        i64p, dp = C.POINTER(C.c_int64), C.POINTER(C.c_double)
        assert lib.abn_sites_sort_keys_dev(gpu_ctx._h, n, *bufs, info.ctypes.data_as(i64p), ms.ctypes.data_as(dp)) == 0
        assert hip.hipMemcpy(order.ctypes.data, bufs[4], 4 * n, 2) == 0
        want, descents, equal = M.reference(k)
        assert np.array_equal(order.astype(np.int64), want)
        assert info.tolist() == [n, descents, equal, 3] and ms[0] > 0.0 and ms[1] > 0.0
        bad = np.array([300], dtype=np.int32)                                # the check kernel finds the key outside its range
        assert hip.hipMemcpy(C.c_void_p(bufs[0].value + 4 * 5), bad.ctypes.data, 4, 1) == 0
        assert lib.abn_sites_sort_keys_dev(gpu_ctx._h, n, *bufs, info.ctypes.data_as(i64p), None) == 1
        assert b"chromosome" in lib.abn_last_error(gpu_ctx._h)
    finally:
        for ptr in bufs:
            hip.hipFree(ptr)


# ---------------------------------------------------------------- the handle
def check_sorted(gpu_ctx, L, name, text, mask, slab_bytes, seen):
    parent, codes = S.resident(gpu_ctx, L, text, mask, slab_bytes)
    child = again = None
    try:
        before, before_ctx, before_flagged = parent.fetch(), parent.contexts(), parent.flagged()
        want = M.reference(M.keys(*(before[k] for k in ("chromosome", "start", "end", "strand"))))
        child = parent.sort()
        got = child.fetch()
        n = len(before["line"])
        for k in KEYS:
            assert got[k].dtype == before[k].dtype and got[k].tobytes() == before[k][want[0]].tobytes(), (name, k)
        assert np.array_equal(got["line"], np.arange(n)), name
        assert child.contexts().tobytes() == before_ctx[want[0]].tobytes(), name
        assert np.array_equal(child.sort_order(), want[0]), name
        rank = np.empty(n, dtype=np.int64)
        rank[want[0]] = np.arange(n)
        flagged_at = np.flatnonzero(np.isin(before["line"], before_flagged))
        assert np.array_equal(child.flagged(), np.sort(rank[flagged_at])), name
        info, cinfo = child.sort_info(), child.info()
        assert (info["sites"], info["descents"], info["equal"]) == (n, want[1], want[2]), name
        assert (cinfo["n_sites"], cinfo["n_lines"], cinfo["n_deferred"]) == (n, n, 0) and child.mask() == mask, name
        assert (info["passes"] == 0) == (want[1] == 0), name
        assert all(m > 0.0 for m in info["ms"]) if n else not info["ms"].any(), (name, info)
        P.assert_sites_equal(parent.fetch(), before, S.KEYS)                               # the parent is not consumed
        again = child.sort()                                                               # a sorted handle sorts to itself
        ainfo = again.sort_info()
        assert (ainfo["descents"], ainfo["passes"]) == (0, 0) and np.array_equal(again.sort_order(), np.arange(n)), name
        P.assert_sites_equal(again.fetch(), got, S.KEYS)
        assert np.array_equal(again.flagged(), child.flagged())
        seen["inserted"] += len(codes)
        seen["flagged"] += len(before_flagged)
        seen["descents"] += want[1]
        if mask == 7:                                                                      # sort then split = split then sort
            a, b = child.split(), parent.split()
            try:
                for ctx_name in a:
                    sorted_kid = b[ctx_name].sort()
                    try:
                        x, y = a[ctx_name].fetch(), sorted_kid.fetch()
                        for k in KEYS:
                            assert x[k].tobytes() == y[k].tobytes(), (name, ctx_name, k)
                        assert a[ctx_name].contexts().tobytes() == sorted_kid.contexts().tobytes()
                        assert len(a[ctx_name].flagged()) == len(sorted_kid.flagged())
                    finally:
                        sorted_kid.close()
            finally:
                for s in list(a.values()) + list(b.values()):
                    s.close()
    finally:
        for s in (again, child, parent):
            if s is not None:
                s.close()


@pytest.mark.parametrize("name", [n for n, _ in SHUFFLED_TEXTS])
@pytest.mark.parametrize("slab_bytes", S.SLABS)
def test_sorted_handle_equals_parent_at_lexsort_order(gpu_ctx, L, slab_bytes, name):
    text = dict(SHUFFLED_TEXTS)[name]
    seen = {"inserted": 0, "flagged": 0, "descents": 0}
    for mask in (1, 7):
        check_sorted(gpu_ctx, L, name, text, mask, slab_bytes, seen)
    if name == "torture":
        assert seen["inserted"] > 0 and seen["flagged"] > 0 and seen["descents"] > 0, seen
    if name == "long row":
        assert seen["inserted"] >= 1, seen
    if name.startswith(("methylome", "plain")):
        assert seen["descents"] > 0, seen


def test_sort_refusals(abn, gpu_ctx):
    lib = gpu_ctx._L
    text = (P.HEADER + "\n".join([P.cg_line(pos="9"), P.cg_line(pos="6", pm="nan"), P.cg_line(pos="7")]) + "\n").encode()

    def parse(entry):
        h, p = C.c_void_p(), abn.SitesParams(0, 1, 1)
        return entry(gpu_ctx._h, text, len(text), C.byref(p), C.byref(h)), h

    out = C.c_void_p(1)
    rc, host_form = parse(lib.abn_sites_parse)
    assert rc == 0 and lib.abn_sites_sort(host_form, C.byref(out)) == 1 and not out.value          # a host-form handle
    rc, r = parse(lib.abn_sites_parse_dev)
    out = C.c_void_p(1)
    assert rc == 0 and lib.abn_sites_sort(r, C.byref(out)) == 1 and not out.value                  # deferred lines pending
    assert b"abn_sites_insert" in lib.abn_last_error(gpu_ctx._h)
    assert lib.abn_sites_sort(None, C.byref(out)) == 1 and lib.abn_sites_sort(r, None) == 1
    n, info = C.c_int64(), np.zeros(4, dtype=np.int64)
    i64p = C.POINTER(C.c_int64)
    assert lib.abn_sites_sort_order(r, C.byref(n), None) == 1                                      # not made by abn_sites_sort
    assert lib.abn_sites_sort_info(r, info.ctypes.data_as(i64p), None) == 1
    assert lib.abn_sites_sort_order(None, None, None) == 1 and lib.abn_sites_sort_info(None, None, None) == 1
    assert lib.abn_sites_insert(r, 0, *[None] * 8) == 0                                            # no deferred line was a site
    assert lib.abn_sites_sort(r, C.byref(out)) == 0 and out.value
    assert lib.abn_sites_sort_order(out, C.byref(n), None) == 0 and n.value == 2
    assert lib.abn_sites_sort_info(out, info.ctypes.data_as(i64p), None) == 0 and info.tolist() == [2, 1, 0, 2]
    for h in (host_form, r, out):
        assert lib.abn_sites_destroy(h) == 0


# ---------------------------------------------------------------- the builders on shuffled golden methylomes
ALIGNS = ("none", "position", "union")


@pytest.fixture(scope="module")
def golden_sets(gpu_ctx):
    """the four golden methylomes with their lines shuffled below the header, parsed and sorted on the device, and the same
    files put in canonical order by the Python model, parsed: made once, shared"""
    texts = [p.read_bytes() for p in P.GOLDEN_METHYLOMES]
    assert len(texts) == 4
    shuffled = [gpu_ctx.parse_sites_resident(M.shuffled_text(t, seed=7 + i), skip_lines=0) for i, t in enumerate(texts)]
    canonical = [gpu_ctx.parse_sites_resident(M.canonical_text(t), skip_lines=0) for t in texts]
    for s in shuffled + canonical:
        assert s.info()["n_deferred"] == 0 and s.info()["n_sites"] == 500
    ordered = [s.sort() for s in shuffled]
    assert all(s.sort_info()["descents"] > 100 for s in ordered)
    yield {"shuffled": shuffled, "sorted": ordered, "canonical": canonical}
    for s in shuffled + canonical + ordered:
        s.close()


def assert_same_arrays(a, b, what):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), what


@pytest.mark.parametrize("align", ALIGNS)
def test_codes_of_sorted_handles_equal_codes_of_canonical_files(abn, gpu_ctx, golden_sets, align):
    a = abn.Codes.from_parsed(gpu_ctx, golden_sets["sorted"], posterior_max_filter=FLT, align=align)
    b = abn.Codes.from_parsed(gpu_ctx, golden_sets["canonical"], posterior_max_filter=FLT, align=align)
    try:
        assert a.info() == b.info() and a.n_sites == 500
        assert_same_arrays(a.stats() + a.pairwise() + (a.packed(), a.transitions()),
                           b.stats() + b.pairwise() + (b.packed(), b.transitions()), align)
    finally:
        a.close(), b.close()


@pytest.mark.parametrize("align", ALIGNS)
def test_tiles_of_sorted_handles_equal_tiles_of_canonical_files(abn, gpu_ctx, golden_sets, align):
    regions = (np.array([1, 1, 2, 256, 257], dtype=np.int32), np.array([0, 1000, 0, 0, 5], dtype=np.int64),
               np.array([500, 1500, 800, 2000, 900], dtype=np.int64), np.array([0, 1, 0, 1, 1], dtype=np.int32))
    for pooled in (False, True):
        a = abn.Tiles.from_parsed(gpu_ctx, golden_sets["sorted"], posterior_max_filter=FLT, align=align)
        b = abn.Tiles.from_parsed(gpu_ctx, golden_sets["canonical"], posterior_max_filter=FLT, align=align)
        try:
            for t in (a, b):
                t.set_pools(*regions, 2) if pooled else t.set_fixed(500)
            assert a.info() == b.info() and a.info()["n_tiles"] == (2 if pooled else a.info()["n_tiles"]) > 1
            assert_same_arrays(a.stats() + a.pairwise() + ((a.pool_columns(),) if pooled else a.layout()),
                               b.stats() + b.pairwise() + ((b.pool_columns(),) if pooled else b.layout()), (align, pooled))
            assert int(a.stats()[0].sum()) > 0
        finally:
            a.close(), b.close()


@pytest.mark.parametrize("align", ALIGNS)
def test_windows_of_sorted_handles_equal_windows_of_canonical_files(abn, gpu_ctx, golden_sets, align):
    import _genes_model as G
    import _windows_model as W

    ann = G.gene_line(1, 500, 1200, "+") + G.gene_line(2, 300, 900, "-") + G.gene_line(5, 800, 1500, "+")
    args = W.Args(cutoff=200, step=5, size=5, absolute=False, flt=FLT)
    kw = dict(cutoff=args.cutoff, cutoff_gene_length=False, step=5, size=5, absolute=False, counts=W.windows_new(args, 100))
    genes = abn.Genes(gpu_ctx, G.gene_lists(W.genome_of(ann)[0]))
    a = abn.Windows.from_parsed(gpu_ctx, genes, golden_sets["sorted"], posterior_max_filter=FLT, align=align, **kw)
    b = abn.Windows.from_parsed(gpu_ctx, genes, golden_sets["canonical"], posterior_max_filter=FLT, align=align, **kw)
    try:
        assert (a.W, a.row_stride, a.n_sites, a.n_samples) == (b.W, b.row_stride, b.n_sites, b.n_samples)
        assert_same_arrays(a.stats() + a.layout() + a.pairwise() + (a.packed(),),
                           b.stats() + b.layout() + b.pairwise() + (b.packed(),), align)
        assert int(a.stats()[0].sum()) > 100
    finally:
        a.close(), b.close(), genes.close()


def test_shuffled_files_are_refused_without_the_sort(abn, gpu_ctx, golden_sets):
    for build in (lambda: abn.Codes.from_parsed(gpu_ctx, golden_sets["shuffled"], posterior_max_filter=FLT, align="position"),
                  lambda: abn.Tiles.from_parsed(gpu_ctx, golden_sets["shuffled"], posterior_max_filter=FLT, align="position")):
        with pytest.raises(abn.AbnError) as e:
            build().close()
        assert e.value.status == 1 and len(str(e.value)) > 20, str(e.value)


# ---------------------------------------------------------------- the tools
@pytest.fixture(scope="module")
def trees(tmp_path_factory):
    """copies of the golden data/ pedigree whose methylomes are shuffled below the header, and put in canonical order"""
    out = {}
    for kind in ("shuffled", "canonical"):
        root = tmp_path_factory.mktemp(kind)
        (root / "data" / "methylome").mkdir(parents=True)
        for f in ("nodelist.txt", "edgelist.txt"):
            (root / "data" / f).write_bytes((GOLDEN / "data" / f).read_bytes())
        for i, p in enumerate(sorted((GOLDEN / "data" / "methylome").glob("*.txt"))):
            text = p.read_bytes()
            (root / "data" / "methylome" / p.name).write_bytes(M.shuffled_text(text, seed=90 + i) if kind == "shuffled"
                                                               else M.canonical_text(text))
        out[kind] = root
    return out


def tool_files(out, names):
    return {f: (out / f).read_bytes() for f in names}


def test_alphabeta_sort_on_shuffled_files_equals_the_run_on_canonical_files(tmp_path, trees):
    runs = {}
    for name, tree, extra in (("want", "canonical", []), ("sorted", "shuffled", ["--sort"]), ("again", "canonical", ["--sort"])):
        out = tmp_path / name
        out.mkdir()
        r = S.run_tool("CLI", *S.ALPHABETA, "-o", out, *extra, cwd=trees[tree])
        assert r.returncode == 0 and "Error" not in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
        runs[name] = (tool_files(out, S.ALPHABETA_FILES), r.stdout)
    assert runs["sorted"][0] == runs["want"][0] and runs["again"][0] == runs["want"][0]
    assert runs["sorted"][1].count("Sorted by position: ") == 4 and " descents\n" in runs["sorted"][1]
    assert "Sorted by position" not in runs["again"][1] and "Sorted by position" not in runs["want"][1]
    r = S.run_tool("CLI", *S.ALPHABETA, "-o", tmp_path, "--align", "position", cwd=trees["shuffled"], timeout=120)
    assert r.returncode == 1 and "Error: " in r.stdout                       # without the sort: today's refusal


def test_metaprofile_tiles_sort_on_shuffled_files_equals_the_run_on_canonical_files(tmp_path, trees):
    common = ["--tiles", "500", "--iterations", "12", "--seed", "99", "--name", "sort"]
    graph = lambda root: ["--methylome", root / "data" / "methylome", "--nodes", root / "data" / "nodelist.txt", "--edges",
                          root / "data" / "edgelist.txt"]
    runs = {}
    for name, tree, extra in (("want", "canonical", []), ("sorted", "shuffled", ["--sort"]), ("again", "canonical", ["--sort"])):
        out = tmp_path / name
        out.mkdir()
        r = S.run_tool("META_CLI", "-o", out, *graph(trees[tree]), *common, *extra, cwd=trees[tree])
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        runs[name] = (tool_files(out, S.TILE_FILES), r.stdout)
    assert runs["sorted"][0] == runs["want"][0] and runs["again"][0] == runs["want"][0]
    assert len(runs["want"][0]["tiles.txt"].splitlines()) > 3
    assert runs["sorted"][1].count("Sorted by position: ") == 4 and "Sorted by position" not in runs["again"][1]


def test_sort_flag_refusals(tmp_path):
    golden = ["-n", "./data/nodelist.txt", "-e", "./data/edgelist.txt", "-o", tmp_path]
    for extra in (["--sort", "--sites", "host"], ["--sort"], ["--sort", "--sites", "device", "--parse", "host"]):
        r = S.run_tool("CLI", *golden, *extra, cwd=GOLDEN, timeout=60)
        assert r.returncode == 2 and "--sort needs --sites device" in r.stderr, (extra, r.stderr)
    meth = GOLDEN / "data" / "methylome"
    tiles = ["-o", tmp_path, "--methylome", meth, "--nodes", GOLDEN / "data" / "nodelist.txt", "--edges",
             GOLDEN / "data" / "edgelist.txt"]
    for args, words in (([*tiles, "--tiles", "50000", "--sort", "--sites", "host"], "--sites host do not apply"),
                        ([*tiles, "--tiles", "50000", "--sort", "--parse", "host"], "--parse host"),
                        (["-o", tmp_path, "--sort"], "not to window directories"),
                        ([*tiles, "--genome", GOLDEN / "annotation.txt", "--sort"], "needs --sites device")):
        r = S.run_tool("META_CLI", *args, cwd=GOLDEN, timeout=60)
        assert r.returncode == 2 and words in r.stderr, (args, r.stderr)
    assert not any(tmp_path.iterdir())
    for tool in ("CLI", "META_CLI"):
        assert "--sort" in S.run_tool(tool, "--help", timeout=60).stdout


def test_metaprofile_tiles_sort_with_contexts_sorts_once_and_splits(tmp_path, trees):
    """--contexts with --sort: the parent is sorted once and then split; the split is stable, so every child is sorted"""
    root = tmp_path / "canonical7"                                           # every context's lines in canonical order
    (root / "data" / "methylome").mkdir(parents=True)
    for f in ("nodelist.txt", "edgelist.txt"):
        (root / "data" / f).write_bytes((GOLDEN / "data" / f).read_bytes())
    for p in sorted((GOLDEN / "data" / "methylome").glob("*.txt")):
        (root / "data" / "methylome" / p.name).write_bytes(M.canonical_text(p.read_bytes(), mask=7))
    common = ["--tiles", "500", "--iterations", "12", "--seed", "99", "--name", "sort", "--contexts", "CG,CHH"]
    graph = lambda r: ["--methylome", r / "data" / "methylome", "--nodes", r / "data" / "nodelist.txt", "--edges",
                       r / "data" / "edgelist.txt"]
    runs = {}
    for name, tree, extra in (("want", root, []), ("sorted", trees["shuffled"], ["--sort"])):
        out = tmp_path / name
        out.mkdir()
        r = S.run_tool("META_CLI", "-o", out, *graph(tree), *common, *extra, cwd=tree)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        runs[name] = {ctx: tool_files(out / ctx, S.TILE_FILES) for ctx in ("CG", "CHH")}
        assert r.stdout.count("Sorted by position: ") == (4 if extra else 0)     # once per methylome, not once per context
    assert runs["sorted"] == runs["want"] and runs["want"]["CG"]["raw.npy"] != runs["want"]["CHH"]["raw.npy"]
