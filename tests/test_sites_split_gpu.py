"""Methylation contexts on the device: the masked device parse (abn_sites_parse, abn_sites_parse_dev with
abn_sites_params.contexts) against the masked host parser, the partition of a resident handle by context (abn_sites_split)
against the single-context parses of the same text, bit for bit, the downstream builders on the children against the same
builders on relabelled files, and the tools' --contexts against their own single-context runs."""
import ctypes as C
import subprocess
from functools import lru_cache
from pathlib import Path

import numpy as np
import pytest

import _contexts_model as X
import _parse_model as P

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden"
FLT = 0.99
KEYS = [k for k, _ in P.FIELDS] + ["status_flag"]
SLABS = (0, 4096, 300)
# a 4-field row beyond the parser's staging limit: the device defers it unread, the host accepts it, and it has no context
LONG_ROW_TEXT = (P.HEADER + P.cg_line(pos="5", ctx="CHG") + "\n" + "chr2\t7\t9\t" + "E" * (P.STAGE + 600) + "\n" +
                 P.cg_line(pos="11", ctx="CHH", st="X") + "\n" + P.cg_line(pos="12") + "\n").encode()
SPLIT_TEXTS = X.texts() + (("long row", LONG_ROW_TEXT), ("rows only", X.rows_only_text(300)),
                           ("header only", P.HEADER.encode()))


@pytest.fixture(scope="module")
def L():
    return X.hostlib()


@lru_cache(maxsize=None)
def host_reference(name, mask):
    """the masked host parser's sites of one of the texts: computed once, shared, never changed"""
    text = dict(SPLIT_TEXTS)[name]
    sites = X.host_sites(X.hostlib(), text, mask)
    for a in sites.values():
        a.setflags(write=False)
    return sites


def merged_by_line(sites, ins):
    """the device's sites and the host-decided lines (X.decide's arrays) as one sequence in file order"""
    names = ("line", "chromosome", "start", "end", "strand", "posteriormax", "status", "meth_lvl", "context")
    both = {k: np.concatenate([sites[k], ins[i]]) for i, k in enumerate(names) if k in sites}
    order = np.argsort(both["line"], kind="stable")
    return {k: v[order] for k, v in both.items()}


def resident(ctx, L, text, mask, slab_bytes):
    """parse_sites_resident under a mask with the host-decided lines inserted -> (handle, the inserted codes)"""
    r = ctx.parse_sites_resident(text, slab_bytes=slab_bytes, contexts=mask)
    ins = X.decide(L, text, r.deferred(), mask)
    r.insert(*ins[:8], context=ins[8])
    return r, ins[8]


# ---------------------------------------------------------------- test 1: the device parse under a mask
@pytest.mark.parametrize("mask", [1, 2, 4, 7])
@pytest.mark.parametrize("slab_bytes", SLABS)
def test_device_parse_equals_masked_host_parser(gpu_ctx, L, slab_bytes, mask):
    assert len(X.texts()) == 9
    for name, text in X.texts():
        want = host_reference(name, mask)
        sites, deferred = gpu_ctx.parse_sites(text, slab_bytes=slab_bytes, contexts=mask)
        ins = X.decide(L, text, deferred, mask)
        if mask == 1:
            assert "context" not in sites
            plain, plain_deferred = gpu_ctx.parse_sites(text, slab_bytes=slab_bytes)       # the no-argument call
            P.assert_sites_equal(sites, plain, KEYS)
            assert sites["n_lines"] == plain["n_lines"]
            assert all(np.array_equal(deferred[k], plain_deferred[k]) for k in deferred), name
        P.assert_sites_equal(merged_by_line(sites, ins), want, [k for k, _ in P.FIELDS] + ["context"] * (mask != 1))
        r = gpu_ctx.parse_sites_resident(text, slab_bytes=slab_bytes, contexts=mask)
        try:
            assert r.mask() == mask
            got = r.deferred()
            assert all(np.array_equal(got[k], deferred[k]) for k in deferred), name
            P.assert_sites_equal(r.fetch(), sites, KEYS)
            r.insert(*ins[:8], context=ins[8])
            P.assert_sites_equal(r.fetch(), want)
            assert r.contexts().tobytes() == want["context"].tobytes(), name
            if mask == 1:
                plain = gpu_ctx.parse_sites_resident(text, slab_bytes=slab_bytes)          # the no-argument call
                try:
                    plain.insert(*ins[:8])
                    P.assert_sites_equal(plain.fetch(), r.fetch(), KEYS)
                    assert np.array_equal(plain.flagged(), r.flagged()) and plain.mask() == 1
                    assert plain.contexts().tobytes() == want["context"].tobytes(), name
                finally:
                    plain.close()
        finally:
            r.close()


def test_golden_counts_on_the_device(gpu_ctx):
    for path in P.GOLDEN_METHYLOMES:
        for mask, n in X.GOLDEN_COUNTS.items():
            sites, deferred = gpu_ctx.parse_sites(path.read_bytes(), contexts=mask)
            assert (len(sites["line"]), len(deferred["line"])) == (n, 0), (path.name, mask)
    names, _ = gpu_ctx.parse_sites(P.GOLDEN_METHYLOMES[0].read_bytes(), contexts=("CHG", "CHH"))
    assert np.bincount(names["context"], minlength=3).tolist() == [0, 400, 1900]


# ---------------------------------------------------------------- test 2: the split
def check_children(gpu_ctx, L, name, text, mask, slab_bytes, seen):
    parent, codes = resident(gpu_ctx, L, text, mask, slab_bytes)
    children = {}
    try:
        before = parent.fetch()
        children = parent.split()
        assert list(children) == [n for c, n in enumerate(X.CONTEXTS) if (mask >> c) & 1], name
        for c, ctx_name in enumerate(X.CONTEXTS):
            if ctx_name not in children:
                continue
            child = children[ctx_name]
            single, single_codes = resident(gpu_ctx, L, text, 1 << c, slab_bytes)
            try:
                want = single.fetch()
                P.assert_sites_equal(child.fetch(), want, KEYS)
                P.assert_sites_equal(want, host_reference(name, 1 << c))                  # and both are the host's parse
                assert child.contexts().tobytes() == single.contexts().tobytes(), (name, ctx_name)
                assert np.array_equal(child.flagged(), single.flagged()), (name, ctx_name)
                info, sinfo = child.info(), single.info()
                assert info["n_deferred"] == 0 and len(child.deferred()["line"]) == 0
                assert (info["n_sites"], info["n_lines"]) == (sinfo["n_sites"], sinfo["n_lines"]), (name, ctx_name)
                assert child.mask() == 1 << c
                seen["inserted"][c] += len(single_codes)
                seen["flagged"][c] += len(single.flagged())
            finally:
                single.close()
        seen["inserted_rows"] += int(np.count_nonzero(codes == 3))
        P.assert_sites_equal(parent.fetch(), before, KEYS)                                 # the parent is not consumed
        again = parent.split()
        try:
            for ctx_name, child in children.items():
                P.assert_sites_equal(again[ctx_name].fetch(), child.fetch(), KEYS)
        finally:
            for s in again.values():
                s.close()
        ms = parent.split_ms()
        n_records = len(before["line"]) - len(codes)
        assert (ms[0] > 0.0 and ms[1] > 0.0) if n_records else ms == (0.0, 0.0), (name, ms)
        assert all(child.split_ms() == children[next(iter(children))].split_ms() for child in children.values())
    finally:
        for s in children.values():
            s.close()
        parent.close()


@pytest.mark.parametrize("name", [n for n, _ in SPLIT_TEXTS])
@pytest.mark.parametrize("slab_bytes", SLABS)
def test_split_equals_single_context_parses(gpu_ctx, L, slab_bytes, name):
    text = dict(SPLIT_TEXTS)[name]
    seen = {"inserted": [0, 0, 0], "flagged": [0, 0, 0], "inserted_rows": 0}
    check_children(gpu_ctx, L, name, text, 7, slab_bytes, seen)
    if name == "torture":
        assert all(n > 0 for n in seen["inserted"]), seen                                  # inserted records in every context
        assert seen["flagged"][1] > 0 and seen["flagged"][2] > 0, seen                     # flagged records outside CG
        for mask in (3, 5, 6):
            check_children(gpu_ctx, L, name, text, mask, slab_bytes, seen)
    if name == "long row":
        assert seen["inserted_rows"] == 1 and seen["inserted"] == [1, 1, 1] and seen["flagged"] == [0, 0, 1], seen
    if name == "rows only":
        check_children(gpu_ctx, L, name, text, 5, slab_bytes, seen)
    if name.startswith("methylome"):
        assert seen["inserted"] == [0, 0, 0]


def test_children_go_into_the_builders_with_their_inserted_lines(abn, gpu_ctx, L):
    """a child's inserted records reach the merge kernels as an ordinary handle's do"""
    text = X.torture_text()
    parent, _ = resident(gpu_ctx, L, text, 7, 4096)
    children = parent.split()
    try:
        for c, name in enumerate(X.CONTEXTS):
            single, codes = resident(gpu_ctx, L, text, 1 << c, 4096)
            assert len(codes) > 0
            a, b = abn.Codes.from_parsed(gpu_ctx, [children[name]], posterior_max_filter=FLT), \
                abn.Codes.from_parsed(gpu_ctx, [single], posterior_max_filter=FLT)
            try:
                assert [x.tobytes() for x in a.stats()] == [y.tobytes() for y in b.stats()], name   # (a NaN level sums to NaN)
                assert a.packed().tobytes() == b.packed().tobytes() and a.n_sites == single.info()["n_sites"]
            finally:
                a.close(), b.close(), single.close()
    finally:
        for s in children.values():
            s.close()
        parent.close()


def test_split_and_contexts_refusals(abn, gpu_ctx):
    lib = gpu_ctx._L
    text = (P.HEADER + "\n".join([P.cg_line(pos="5"), P.cg_line(pos="6", ctx="CHG", pm="nan"), P.cg_line(pos="7", ctx="CHH")]) +
            "\n").encode()

    def parse(entry, contexts, text=text):
        h, p = C.c_void_p(), abn.SitesParams(0, 1, contexts)
        return entry(gpu_ctx._h, text, len(text), C.byref(p), C.byref(h)), h

    for entry in (lib.abn_sites_parse, lib.abn_sites_parse_dev):
        for bad in (8, -1, 1 << 20):
            rc, h = parse(entry, bad)
            assert rc == 1 and not h.value
    out = (C.c_void_p * 3)(1, 1, 1)
    rc, host_form = parse(lib.abn_sites_parse, 7)
    assert rc == 0 and lib.abn_sites_split(host_form, out) == 1 and list(out) == [None] * 3       # a host-form handle
    mask, codes = C.c_int32(), np.zeros(2, dtype=np.uint8)
    assert lib.abn_sites_context(host_form, C.byref(mask), codes.ctypes.data_as(C.POINTER(C.c_uint8))) == 0
    assert mask.value == 7 and codes.tolist() == [0, 2]
    rc, r = parse(lib.abn_sites_parse_dev, 7)
    assert rc == 0
    assert lib.abn_sites_split(r, out) == 1 and list(out) == [None] * 3                            # deferred lines pending
    assert lib.abn_sites_split(None, out) == 1 and lib.abn_sites_split(r, None) == 1
    assert lib.abn_sites_split_ms(None, None) == 1 and lib.abn_sites_context(None, None, None) == 1
    one = [np.array(v, dtype=t) for v, t in zip(([2], [1], [6], [7], [0], [np.nan], [2], [0.5]),
                                                (np.int64, np.int32, np.uint32, np.uint32, np.uint8, np.float64, np.uint8, np.float64))]
    args = [a.ctypes.data_as(t) for a, t in zip(one, lib.abn_sites_insert.argtypes[2:])]
    code = lambda v: np.array([v], dtype=np.uint8).ctypes.data_as(C.POINTER(C.c_uint8))
    assert lib.abn_sites_insert(r, 1, *args) == 1                                                  # CG codes into a mask-7 handle
    assert lib.abn_sites_insert_ctx(r, 1, *args, code(4)) == 1 and lib.abn_sites_insert_ctx(r, 1, *args, None) == 1
    assert lib.abn_sites_insert_ctx(r, 1, *args, code(1)) == 0
    assert lib.abn_sites_split(r, out) == 0 and all(out)
    for h in out:
        assert lib.abn_sites_destroy(h) == 0
    rc, two = parse(lib.abn_sites_parse_dev, 5)
    assert rc == 0 and lib.abn_sites_insert_ctx(two, 0, *[None] * 9) == 0                          # nothing deferred under CG + CHH
    rc, pending = parse(lib.abn_sites_parse_dev, 2)
    assert rc == 0 and lib.abn_sites_insert_ctx(pending, 1, *args, code(0)) == 1                   # a code outside the mask
    assert lib.abn_sites_insert_ctx(pending, 1, *args, code(3)) == 0                               # a row without one is in every mask
    for h in (host_form, r, two, pending):
        assert lib.abn_sites_destroy(h) == 0


# ---------------------------------------------------------------- test 3: the builders on the children
@pytest.fixture(scope="module")
def golden_children(gpu_ctx):
    """the four golden methylomes parsed once under every context (skip_lines 0, as the pedigree build reads them) and
    split, and the same files relabelled per context and parsed with no contexts argument"""
    texts = [p.read_bytes() for p in P.GOLDEN_METHYLOMES]
    parents = [gpu_ctx.parse_sites_resident(t, skip_lines=0, contexts=X.CONTEXTS) for t in texts]
    for p in parents:
        assert p.info()["n_deferred"] == 0
    children = [p.split() for p in parents]
    relabelled = {name: [gpu_ctx.parse_sites_resident(X.relabel(t, c), skip_lines=0) for t in texts]
                  for c, name in enumerate(X.CONTEXTS)}
    yield children, relabelled
    for s in parents + [s for d in children for s in d.values()] + [s for l in relabelled.values() for s in l]:
        s.close()


@pytest.mark.parametrize("name", X.CONTEXTS)
def test_codes_of_children_equal_codes_of_relabelled_files(abn, gpu_ctx, golden_children, name):
    children, relabelled = golden_children
    a = abn.Codes.from_parsed(gpu_ctx, [d[name] for d in children], posterior_max_filter=FLT)
    b = abn.Codes.from_parsed(gpu_ctx, relabelled[name], posterior_max_filter=FLT)
    try:
        assert a.info() == b.info() and a.n_sites == {"CG": 500, "CHG": 400, "CHH": 1900}[name]
        for x, y in zip(a.stats() + a.pairwise(), b.stats() + b.pairwise()):
            assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), name
        assert a.packed().tobytes() == b.packed().tobytes()
        assert int(a.stats()[2].min()) > 0
    finally:
        a.close(), b.close()


@pytest.mark.parametrize("name", X.CONTEXTS)
def test_tiles_of_children_equal_tiles_of_relabelled_files(abn, gpu_ctx, golden_children, name):
    children, relabelled = golden_children
    a = abn.Tiles.from_parsed(gpu_ctx, [d[name] for d in children], posterior_max_filter=FLT)
    b = abn.Tiles.from_parsed(gpu_ctx, relabelled[name], posterior_max_filter=FLT)
    try:
        a.set_fixed(50000), b.set_fixed(50000)
        assert a.info() == b.info() and a.info()["n_tiles"] > 1
        for x, y in zip(a.stats() + a.pairwise() + a.layout(), b.stats() + b.pairwise() + b.layout()):
            assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), name
    finally:
        a.close(), b.close()


# ---------------------------------------------------------------- test 4: the tools
def run_tool(tool, *args, cwd=None, timeout=300):
    from alphabeta_rs_amd import build as B

    B.build_host()
    return subprocess.run([str(getattr(B, tool)), *map(str, args)], capture_output=True, text=True, timeout=timeout, cwd=cwd)


@pytest.fixture(scope="module")
def relabelled_trees(tmp_path_factory):
    """per context a copy of the golden data/ pedigree whose methylomes are relabelled: the tools without --contexts read
    on it what --contexts <that context> reads on the golden files"""
    trees = {}
    for c, name in enumerate(X.CONTEXTS):
        root = tmp_path_factory.mktemp("relabelled_" + name)
        (root / "data" / "methylome").mkdir(parents=True)
        for f in ("nodelist.txt", "edgelist.txt"):
            (root / "data" / f).write_bytes((GOLDEN / "data" / f).read_bytes())
        for p in sorted((GOLDEN / "data" / "methylome").glob("*.txt")):
            (root / "data" / "methylome" / p.name).write_bytes(X.relabel(p.read_bytes(), c))
        trees[name] = root
    return trees


ALPHABETA = ["-i", "20", "--seed", "4711", "-n", "./data/nodelist.txt", "-e", "./data/edgelist.txt", "--sites", "device"]
ALPHABETA_FILES = ("pedigree.txt", "analysis.txt", "raw.npy")


def test_alphabeta_contexts_equal_runs_on_relabelled_files(tmp_path, relabelled_trees):
    want = {}
    for name in X.CONTEXTS:                                                  # no --contexts, the relabelled copies
        out = tmp_path / ("want_" + name)
        out.mkdir()
        r = run_tool("CLI", *ALPHABETA, "-o", out, cwd=relabelled_trees[name])
        assert r.returncode == 0 and "Error" not in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
        want[name] = {f: (out / f).read_bytes() for f in ALPHABETA_FILES}
    assert len({v["raw.npy"] for v in want.values()}) == 3                   # three different fits
    today = tmp_path / "today"
    today.mkdir()
    r = run_tool("CLI", *ALPHABETA, "-o", today, cwd=GOLDEN)                  # today's run: the golden files, no option
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert {f: (today / f).read_bytes() for f in ALPHABETA_FILES} == want["CG"]
    for name in ("CHG", "CG"):                                               # one context: the same files in the same place
        out = tmp_path / ("one_" + name)
        out.mkdir()
        r = run_tool("CLI", *ALPHABETA, "-o", out, "--contexts", name, cwd=GOLDEN)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        assert {f: (out / f).read_bytes() for f in ALPHABETA_FILES} == want[name], name
        assert sorted(p.name for p in out.iterdir()) == sorted(ALPHABETA_FILES)
    out = tmp_path / "all"                                                   # several: one parse, a subdirectory each
    out.mkdir()
    r = run_tool("CLI", *ALPHABETA, "-o", out, "--contexts", "CG,CHG,CHH", cwd=GOLDEN)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert sorted(p.name for p in out.iterdir()) == ["CG", "CHG", "CHH"]
    for name in X.CONTEXTS:
        assert {f: (out / name / f).read_bytes() for f in ALPHABETA_FILES} == want[name], name
    out = tmp_path / "two"                                                   # the list's order does not matter
    out.mkdir()
    r = run_tool("CLI", *ALPHABETA, "-o", out, "--contexts=CHH,CG", cwd=GOLDEN)
    assert r.returncode == 0 and sorted(p.name for p in out.iterdir()) == ["CG", "CHH"]
    for name in ("CG", "CHH"):
        assert {f: (out / name / f).read_bytes() for f in ALPHABETA_FILES} == want[name], name


TILE_FILES = ("results.txt", "raw.npy", "tiles.txt")


def test_metaprofile_tiles_contexts_equal_runs_on_relabelled_files(tmp_path, relabelled_trees):
    common = ["--tiles", "50000", "--iterations", "12", "--seed", "99", "--name", "ctx"]
    graph = lambda root: ["--methylome", root / "data" / "methylome", "--nodes", root / "data" / "nodelist.txt", "--edges",
                          root / "data" / "edgelist.txt"]
    want = {}
    for name in ("CG", "CHH"):
        out = tmp_path / ("want_" + name)
        out.mkdir()
        r = run_tool("META_CLI", "-o", out, *graph(relabelled_trees[name]), *common, cwd=relabelled_trees[name])
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        want[name] = {f: (out / f).read_bytes() for f in TILE_FILES}
        listed = [l.split(";") for l in (out / "tiles.txt").read_text().splitlines()[1:]]
        fitted = [l for l in listed if l[5] == "1"]
        assert len(fitted) >= 1 and len(fitted) + r.stdout.count("Error: Error while building pedigree: tile") == len(listed)
    assert want["CG"]["raw.npy"] != want["CHH"]["raw.npy"]
    out = tmp_path / "both"
    out.mkdir()
    r = run_tool("META_CLI", "-o", out, *graph(GOLDEN), *common, "--contexts", "CG,CHH", cwd=GOLDEN)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert sorted(p.name for p in out.iterdir()) == ["CG", "CHH"]
    for name in ("CG", "CHH"):
        assert {f: (out / name / f).read_bytes() for f in TILE_FILES} == want[name], name
    one = tmp_path / "one"
    one.mkdir()
    r = run_tool("META_CLI", "-o", one, *graph(GOLDEN), *common, "--contexts", "CHH", cwd=GOLDEN)
    assert r.returncode == 0 and {f: (one / f).read_bytes() for f in TILE_FILES} == want["CHH"]


def test_contexts_flag_refusals(tmp_path):
    golden = ["-n", "./data/nodelist.txt", "-e", "./data/edgelist.txt", "-o", tmp_path]
    for extra, words in ((["--contexts", "CHG", "--sites", "host"], "--contexts needs --sites device"),
                         (["--contexts", "CHG"], "--contexts needs --sites device"),
                         (["--contexts", "CHG", "--sites", "device", "--parse", "host"], "--contexts needs --sites device and --parse device"),
                         (["--contexts", "CG,CH", "--sites", "device"], "--contexts expects"),
                         (["--contexts", "CG,CG", "--sites", "device"], "--contexts expects"),
                         (["--contexts", "", "--sites", "device"], "--contexts expects")):
        r = run_tool("CLI", *golden, *extra, cwd=GOLDEN, timeout=60)
        assert r.returncode != 0 and words in r.stderr, (extra, r.stderr)
    meth = GOLDEN / "data" / "methylome"
    tiles = ["-o", tmp_path, "--methylome", meth, "--nodes", GOLDEN / "data" / "nodelist.txt", "--edges",
             GOLDEN / "data" / "edgelist.txt"]
    for args, words in (([*tiles, "--tiles", "50000", "--contexts", "CHG", "--sites", "host"], "--sites host do not apply"),
                        ([*tiles, "--tiles", "50000", "--contexts", "CHG", "--parse", "host"], "--parse host"),
                        (["-o", tmp_path, "--contexts", "CHG"], "not to window directories"),
                        ([*tiles, "--genome", GOLDEN / "annotation.txt", "--contexts", "CHG"], "not to the gene windows of --genome"),
                        ([*tiles, "--tiles", "50000", "--contexts", "CHG,XX"], "--contexts expects"),
                        ([*tiles, "--tiles", "50000", "--contexts", "CHH,CHH"], "--contexts expects")):
        r = run_tool("META_CLI", *args, cwd=GOLDEN, timeout=60)
        assert r.returncode != 0 and words in r.stderr, (args, r.stderr)
    assert not any(tmp_path.iterdir())
    for tool in ("CLI", "META_CLI"):
        assert "--contexts" in run_tool(tool, "--help", timeout=60).stdout
