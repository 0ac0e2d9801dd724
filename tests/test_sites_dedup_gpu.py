"""The collapse of repeated sites of resident methylomes on the device (abn_sites_dedup, abn_sites_dedup_keys): the
primitive on raw arrays and the collapsed handle against the numpy / Python model of tests/_dedup_model.py — never the code
under test — exactly; the builders on dedup(sort(doubled file)) against the same builders on sort(original file), byte
for byte; and the tools' --dedup."""
import ctypes as C
from functools import lru_cache
from pathlib import Path

import numpy as np
import pytest

import _dedup_model as M
import _parse_model as P
import test_sites_split_gpu as S   # its texts and helpers, as they are

from alphabeta_rs_amd import dedup as D

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden"
FLT = 0.99
KEYS = [k for k in S.KEYS if k != "line"]
PATTERNS = ("no repeats", "all equal", "pairs", "random runs", "all-NaN runs", "straddling", "start and end", "long run")
DOUBLED_TEXTS = tuple((name, *M.doubled_text(text, seed=61 + i, skip_lines=1)) for i, (name, text) in enumerate(S.SPLIT_TEXTS))


# ---------------------------------------------------------------- the primitive
@lru_cache(maxsize=None)
def cases():
    """(n, pattern name, records, {policy: the model's (order, info4)}) of every primitive case, made once"""
    out = []
    for n in M.SIZES:
        for name, r in M.patterns(n, seed=n):
            for a in r:
                a.setflags(write=False)
            out.append((n, name, r, {policy: M.model(r, policy) for policy in M.POLICIES}))
    return tuple(out)


def test_primitive_cases_cover_the_sizes_and_patterns():
    assert M.SIZES == (0, 1, 2, 63, 64, 65, 2047, 2048, 2049, 3 * 2048 + 17)
    assert {name for _, name, _, _ in cases()} == set(PATTERNS)
    assert sum(1 for n, name, _, _ in cases() if name == "long run") == 1 and M.LONG_RUN == 2 * 2048 + 5


@pytest.mark.parametrize("policy", M.POLICIES)
@pytest.mark.parametrize("pattern", PATTERNS)
def test_primitive_equals_the_model(gpu_ctx, pattern, policy):
    for n, name, r, want in cases():
        if name != pattern:
            continue
        order, info = D.dedup_sites(gpu_ctx, *r, policy=policy)
        assert order.dtype == np.int64 and np.array_equal(order, want[policy][0]), (n, name, policy)
        assert [info["sites"], info["kept"], info["repeated"], info["disagreeing"]] == want[policy][1], (n, name, policy)


def test_primitive_refusals(abn, gpu_ctx):
    lib = gpu_ctx._L
    ok = M.records([1, 1], [5, 5], [6, 6], [0, 0], [0.5, 0.7], [0, 2])
    for bad in ((258, 0, 0, 0), (-1, 0, 0, 0), (0, 0, 0, 3)):
        with pytest.raises(abn.AbnError) as e:
            D.dedup_sites(gpu_ctx, *([0, v] for v in bad), [0.5, 0.5], [0, 0])
        assert e.value.status == 1
    with pytest.raises(abn.AbnError) as e:                                    # a descent: named, and the remedy
        D.dedup_sites(gpu_ctx, [1, 1, 0], [5, 5, 9], [6, 6, 10], [0, 0, 0], [0.5] * 3, [0] * 3, policy="best")
    assert e.value.status == 1 and "site 2" in str(e.value) and "sort first" in str(e.value)
    with pytest.raises(ValueError):
        D.dedup_sites(gpu_ctx, *ok, policy="newest")
    for policy in (-1, 4):
        with pytest.raises(abn.AbnError):
            D.dedup_sites(gpu_ctx, *ok, policy=policy)
    info, order = np.zeros(4, dtype=np.int64), np.zeros(2, dtype=np.int64)
    i64p = C.POINTER(C.c_int64)
    ip, op = info.ctypes.data_as(i64p), order.ctypes.data_as(i64p)
    nulls = [None] * 6
    assert lib.abn_sites_dedup_keys(gpu_ctx._h, 1, *nulls, 0, op, ip) == 1
    assert lib.abn_sites_dedup_keys(gpu_ctx._h, 0, *nulls, 0, None, None) == 1
    assert lib.abn_sites_dedup_keys(gpu_ctx._h, 1 << 32, *nulls, 0, op, ip) == 1
    assert lib.abn_sites_dedup_keys(None, 0, *nulls, 0, None, ip) == 1
    assert lib.abn_sites_dedup_keys(gpu_ctx._h, 0, *nulls, 0, None, ip) == 0 and info.tolist() == [0, 0, 0, 0]
    assert lib.abn_sites_dedup_keys_dev(gpu_ctx._h, 1, *nulls, 0, None, ip, None) == 1
    assert lib.abn_sites_dedup_keys_dev(gpu_ctx._h, 0, *nulls, 4, None, ip, None) == 1
    assert lib.abn_sites_dedup_keys_dev(gpu_ctx._h, 0, *nulls, 0, None, ip, None) == 0


def test_primitive_on_device_arrays(gpu_ctx):
    """Records and order stay in HBM.  The device buffers come from the HIP runtime the product library already holds, as
    in tests/test_sites_sort_gpu.py::test_primitive_on_device_arrays.  A planted descent and a planted bad key are found
    by the flags kernel and refused."""
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipFree.argtypes = [C.c_void_p]
    lib = gpu_ctx._L
    n, name, r, want = next(c for c in cases() if c[0] == 3 * 2048 + 17 and c[1] == "random runs")
    bufs = [C.c_void_p() for _ in range(7)]
    for ptr, size in zip(bufs, (4 * n, 4 * n, 4 * n, n, 8 * n, n, 4 * n)):
        assert hip.hipMalloc(C.byref(ptr), size) == 0
    try:
        for ptr, a in zip(bufs, r):
            assert hip.hipMemcpy(ptr, a.ctypes.data, a.nbytes, 1) == 0
        i64p, dp = C.POINTER(C.c_int64), C.POINTER(C.c_double)
        for k, policy in enumerate(M.POLICIES):
            info, ms, order = np.zeros(4, dtype=np.int64), np.zeros(2), np.zeros(n, dtype=np.uint32)
            assert lib.abn_sites_dedup_keys_dev(gpu_ctx._h, n, *bufs[:6], k, bufs[6], info.ctypes.data_as(i64p),
                                                ms.ctypes.data_as(dp)) == 0
            assert hip.hipMemcpy(order.ctypes.data, bufs[6], 4 * n, 2) == 0
            assert info.tolist() == want[policy][1] and ms[0] > 0.0 and ms[1] > 0.0, policy
            assert np.array_equal(order[:info[1]].astype(np.int64), want[policy][0]), policy
        info = np.zeros(4, dtype=np.int64)
        low = np.array([0], dtype=np.uint32)                                 # a planted descent: start 0 behind start > 0
        assert hip.hipMemcpy(C.c_void_p(bufs[1].value + 4 * 4000), low.ctypes.data, 4, 1) == 0
        assert lib.abn_sites_dedup_keys_dev(gpu_ctx._h, n, *bufs[:6], 2, bufs[6], info.ctypes.data_as(i64p), None) == 1
        err = lib.abn_last_error(gpu_ctx._h)
        assert b"site 4000 " in err and b"sort first" in err, err
        assert hip.hipMemcpy(C.c_void_p(bufs[1].value + 4 * 4000), r[1][4000:].ctypes.data, 4, 1) == 0
        bad = np.array([300], dtype=np.int32)                                # a planted key outside its range
        assert hip.hipMemcpy(C.c_void_p(bufs[0].value + 4 * 5), bad.ctypes.data, 4, 1) == 0
        assert lib.abn_sites_dedup_keys_dev(gpu_ctx._h, n, *bufs[:6], 0, bufs[6], info.ctypes.data_as(i64p), None) == 1
        assert b"chromosome" in lib.abn_last_error(gpu_ctx._h)
    finally:
        for ptr in bufs:
            hip.hipFree(ptr)


# ---------------------------------------------------------------- the handle
def check_collapsed(gpu_ctx, L, name, text, copies, mask, slab_bytes, seen):
    raw, codes = S.resident(gpu_ctx, L, text, mask, slab_bytes)
    parent = raw.sort()
    kids = []
    try:
        before, before_ctx, before_flagged = parent.fetch(), parent.contexts(), parent.flagged()
        r = M.fetch_records(before)
        assert M.first_descent(r) == -1
        for policy in M.POLICIES:
            want, winfo = M.model(r, policy)
            child = D.dedup(parent, policy)
            kids.append(child)
            got, n = child.fetch(), len(want)
            for k in KEYS:
                assert got[k].dtype == before[k].dtype and got[k].tobytes() == before[k][want].tobytes(), (name, policy, k)
            assert np.array_equal(got["line"], np.arange(n)), (name, policy)
            assert child.contexts().tobytes() == before_ctx[want].tobytes(), (name, policy)
            order = D.dedup_order(child)
            assert np.array_equal(order, want) and (np.diff(order) > 0).all(), (name, policy)
            flagged_at = np.flatnonzero(np.isin(before["line"], before_flagged))
            assert np.array_equal(child.flagged(), np.flatnonzero(np.isin(want, flagged_at))), (name, policy)
            info, cinfo = D.dedup_info(child), child.info()
            assert [info["sites"], info["kept"], info["repeated"], info["disagreeing"]] == winfo, (name, policy)
            assert (cinfo["n_sites"], cinfo["n_lines"], cinfo["n_deferred"]) == (n, n, 0) and child.mask() == mask, (name, policy)
            assert (info["ms"][:3] > 0.0).all() if len(r[0]) else not info["ms"].any(), (name, info)
            if mask == 1 and name.startswith(("methylome", "plain")):            # every CG site stands twice, its status changed
                assert winfo[3] == winfo[2] == seen["doubled"][name] > 0, (name, winfo, seen)
            if mask == 7:                                                        # the split of the child = the split of the model's records
                ctx_of = before_ctx[want]
                for ctx_name, kid in child.split().items():
                    try:
                        pick = want[(ctx_of == S.X.CONTEXTS.index(ctx_name)) | (ctx_of == 3)]   # a row without a context: every child's
                        x = kid.fetch()
                        for k in KEYS:
                            assert x[k].tobytes() == before[k][pick].tobytes(), (name, policy, ctx_name, k)
                    finally:
                        kid.close()
        P.assert_sites_equal(parent.fetch(), before, S.KEYS)                       # the parent is not consumed
        seen["inserted"] += len(codes)
        seen["flagged"] += len(before_flagged)
        seen["repeated"] += winfo[2]
    finally:
        for s in kids + [parent, raw]:
            s.close()


@pytest.mark.parametrize("name", [n for n, _, _ in DOUBLED_TEXTS])
def test_collapsed_handle_equals_the_model_on_the_sorted_parent(gpu_ctx, name):
    L = S.X.hostlib()
    text, copies = next((t, c) for n, t, c in DOUBLED_TEXTS if n == name)
    seen = {"inserted": 0, "flagged": 0, "repeated": 0, "doubled": {}}
    if name.startswith(("methylome", "plain")):
        seen["doubled"][name] = len(S.X.host_sites(L, dict(S.SPLIT_TEXTS)[name], 1)["line"])
    for mask, slab_bytes in ((1, 300), (7, 4096), (7, 300)):
        check_collapsed(gpu_ctx, L, name, text, copies, mask, slab_bytes, seen)
    if name == "torture":
        assert seen["inserted"] > 0 and seen["flagged"] > 0 and seen["repeated"] > 0, seen
    if name.startswith(("methylome", "plain")):
        assert seen["repeated"] > 0 and copies > 0, seen


def test_dedup_refusals(abn, gpu_ctx):
    lib = gpu_ctx._L
    text = (P.HEADER + "\n".join([P.cg_line(pos="9"), P.cg_line(pos="6", pm="nan"), P.cg_line(pos="7"), P.cg_line(pos="7")]) +
            "\n").encode()

    def parse(entry):
        h, p = C.c_void_p(), abn.SitesParams(0, 1, 1)
        return entry(gpu_ctx._h, text, len(text), C.byref(p), C.byref(h)), h

    out = C.c_void_p(1)
    rc, host_form = parse(lib.abn_sites_parse)
    assert rc == 0 and lib.abn_sites_dedup(host_form, 0, C.byref(out)) == 1 and not out.value       # a host-form handle
    rc, r = parse(lib.abn_sites_parse_dev)
    out = C.c_void_p(1)
    assert rc == 0 and lib.abn_sites_dedup(r, 0, C.byref(out)) == 1 and not out.value               # deferred lines pending
    assert b"abn_sites_insert" in lib.abn_last_error(gpu_ctx._h)
    assert lib.abn_sites_dedup(None, 0, C.byref(out)) == 1 and lib.abn_sites_dedup(r, 0, None) == 1
    assert lib.abn_sites_insert(r, 0, *[None] * 8) == 0                                            # no deferred line was a site
    for policy in (-1, 4):
        out = C.c_void_p(1)
        assert lib.abn_sites_dedup(r, policy, C.byref(out)) == 1 and not out.value
        assert b"policy" in lib.abn_last_error(gpu_ctx._h)
    out = C.c_void_p(1)
    assert lib.abn_sites_dedup(r, 0, C.byref(out)) == 1 and not out.value                          # an unsorted parent
    err = lib.abn_last_error(gpu_ctx._h)
    assert b"site 1 " in err and b"sort first" in err, err
    n, info = C.c_int64(), np.zeros(4, dtype=np.int64)
    i64p = C.POINTER(C.c_int64)
    ordered = C.c_void_p()
    assert lib.abn_sites_sort(r, C.byref(ordered)) == 0
    for h in (r, ordered):                                                                         # not made by abn_sites_dedup
        assert lib.abn_sites_dedup_order(h, C.byref(n), None) == 1
        assert lib.abn_sites_dedup_info(h, info.ctypes.data_as(i64p), None) == 1
    assert lib.abn_sites_dedup_order(None, None, None) == 1 and lib.abn_sites_dedup_info(None, None, None) == 1
    assert lib.abn_sites_dedup(ordered, 3, C.byref(out)) == 0 and out.value
    assert lib.abn_sites_dedup_order(out, C.byref(n), None) == 0 and n.value == 1
    assert lib.abn_sites_dedup_info(out, info.ctypes.data_as(i64p), None) == 0 and info.tolist() == [3, 1, 1, 0]
    assert lib.abn_sites_sort_order(out, C.byref(n), None) == 1                                    # nor is it a sort's child
    for h in (host_form, r, ordered, out):
        assert lib.abn_sites_destroy(h) == 0


# ---------------------------------------------------------------- the builders on doubled golden methylomes
ALIGNS = ("none", "position", "union")


def subset_of(text):
    """the lines below the header, by index, that hold every seventh CG site of a golden methylome"""
    cg = [k for k, line in enumerate(text.split(b"\n")[1:]) if line.split(b"\t")[3:4] == [b"CG"]]
    return set(cg[::7])


@pytest.fixture(scope="module")
def golden_sets(gpu_ctx):
    """The four golden methylomes sorted on the device, and their doubled texts sorted and collapsed: shuffled for `best`
    (every copy has the lower posteriormax), every copy behind its original for `first`; for `drop` only the lines of
    subset_of(text) are doubled, against the original files without those lines.  Made once, shared."""
    texts = [p.read_bytes() for p in P.GOLDEN_METHYLOMES]
    assert len(texts) == 4
    made = []

    def handles(variants, policy=None):
        out = []
        for t in variants:
            raw = gpu_ctx.parse_sites_resident(t, skip_lines=0)
            assert raw.info()["n_deferred"] == 0
            ordered = raw.sort()
            made.extend([raw, ordered])
            if policy is None:
                out.append(ordered)
            else:
                out.append(D.dedup(ordered, policy))
                made.append(out[-1])
        return out

    sets = {"original": handles(texts),
            "best": handles([M.doubled_text(t, seed=17 + i, skip_lines=1)[0] for i, t in enumerate(texts)], "best"),
            "first": handles([M.doubled_text(t, skip_lines=1)[0] for t in texts], "first"),
            "drop": handles([M.doubled_text(t, seed=29 + i, skip_lines=1, subset=subset_of(t))[0] for i, t in enumerate(texts)],
                            "drop"),
            "without": handles([b"".join(l for k, l in enumerate(t.splitlines(keepends=True)) if k == 0 or k - 1 not in subset_of(t))
                                for t in texts])}
    for s in sets["original"]:
        assert s.info()["n_sites"] == 500 and (s.fetch()["posteriormax"] > 0).all()
    for policy in ("best", "first"):
        for s in sets[policy]:
            i = D.dedup_info(s)
            assert (i["sites"], i["kept"], i["repeated"], i["disagreeing"]) == (1000, 500, 500, 500)
    for s, w in zip(sets["drop"], sets["without"]):
        i, left = D.dedup_info(s), w.info()["n_sites"]
        assert left == 500 - 72 and (i["sites"], i["kept"], i["repeated"]) == (500 + 72, left, 72)
    yield sets
    for s in made:
        s.close()


def assert_same_arrays(a, b, what):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), what


@pytest.mark.parametrize("align", ALIGNS)
@pytest.mark.parametrize("policy, against", [("best", "original"), ("first", "original"), ("drop", "without")])
def test_codes_of_collapsed_handles_equal_codes_of_the_original_files(abn, gpu_ctx, golden_sets, policy, against, align):
    a = abn.Codes.from_parsed(gpu_ctx, golden_sets[policy], posterior_max_filter=FLT, align=align)
    b = abn.Codes.from_parsed(gpu_ctx, golden_sets[against], posterior_max_filter=FLT, align=align)
    try:
        assert a.info() == b.info() and a.n_sites == b.n_sites > 300            # (the samples do not share every site)
        assert_same_arrays(a.stats() + a.pairwise() + (a.packed(),), b.stats() + b.pairwise() + (b.packed(),), (policy, align))
    finally:
        a.close(), b.close()


@pytest.mark.parametrize("policy, against", [("best", "original"), ("first", "original"), ("drop", "without")])
def test_tiles_of_collapsed_handles_equal_tiles_of_the_original_files(abn, gpu_ctx, golden_sets, policy, against):
    a = abn.Tiles.from_parsed(gpu_ctx, golden_sets[policy], posterior_max_filter=FLT, align="position")
    b = abn.Tiles.from_parsed(gpu_ctx, golden_sets[against], posterior_max_filter=FLT, align="position")
    try:
        for t in (a, b):
            t.set_fixed(500)
        assert a.info() == b.info() and a.info()["n_tiles"] > 1
        assert_same_arrays(a.stats() + a.pairwise() + a.layout(), b.stats() + b.pairwise() + b.layout(), policy)
        assert int(a.stats()[0].sum()) > 0
    finally:
        a.close(), b.close()


# ---------------------------------------------------------------- the tools
@pytest.fixture(scope="module")
def trees(tmp_path_factory):
    """copies of the golden data/ pedigree: the original methylomes; every site line doubled and the lines shuffled; every
    site line doubled, each copy behind its original"""
    out = {}
    for kind in ("original", "doubled shuffled", "doubled in order"):
        root = tmp_path_factory.mktemp(kind.replace(" ", "_"))
        (root / "data" / "methylome").mkdir(parents=True)
        for f in ("nodelist.txt", "edgelist.txt"):
            (root / "data" / f).write_bytes((GOLDEN / "data" / f).read_bytes())
        for i, p in enumerate(sorted((GOLDEN / "data" / "methylome").glob("*.txt"))):
            text = p.read_bytes()
            if kind != "original":
                text = M.doubled_text(text, seed=70 + i if kind == "doubled shuffled" else None, skip_lines=1)[0]
            (root / "data" / "methylome" / p.name).write_bytes(text)
        out[kind] = root
    return out


def tool_files(out, names):
    return {f: (out / f).read_bytes() for f in names}


def test_alphabeta_dedup_on_doubled_files_equals_the_sorted_run_on_the_original_files(tmp_path, trees):
    runs = {}
    for name, tree, extra in (("want", "original", ["--sort"]), ("best", "doubled shuffled", ["--dedup", "best"]),
                              ("plain", "original", ["--dedup", "best"])):
        out = tmp_path / name
        out.mkdir()
        r = S.run_tool("CLI", *S.ALPHABETA, "-o", out, "--align", "position", *extra, cwd=trees[tree])
        assert r.returncode == 0 and "Error" not in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
        runs[name] = (tool_files(out, S.ALPHABETA_FILES), r.stdout)
    assert runs["best"][0] == runs["want"][0] and runs["plain"][0] == runs["want"][0]
    assert runs["best"][1].count("Collapsed repeated sites: ") == 4 and " disagreeing (best)\n" in runs["best"][1]
    assert runs["best"][1].count("Sorted by position: ") == 4                  # --dedup implies the sort
    assert "Collapsed" not in runs["plain"][1] and "Collapsed" not in runs["want"][1]


def test_the_doubled_files_are_refused_without_dedup(tmp_path, trees):
    """today's gap, which --dedup closes: behind the sort the repeated keys are adjacent, and the alignment refuses them"""
    r = S.run_tool("CLI", *S.ALPHABETA, "-o", tmp_path, "--sort", "--align", "position", cwd=trees["doubled shuffled"], timeout=120)
    assert r.returncode == 1 and "Error: " in r.stdout and "ascending" in r.stdout, r.stdout[-2000:]


def test_metaprofile_tiles_dedup_on_doubled_files_equals_the_sorted_run_on_the_original_files(tmp_path, trees):
    common = ["--tiles", "500", "--iterations", "12", "--seed", "99", "--name", "dedup"]
    graph = lambda root: ["--methylome", root / "data" / "methylome", "--nodes", root / "data" / "nodelist.txt", "--edges",
                          root / "data" / "edgelist.txt"]
    runs = {}
    for name, tree, extra in (("want", "original", ["--sort"]), ("first", "doubled in order", ["--dedup", "first"])):
        out = tmp_path / name
        out.mkdir()
        r = S.run_tool("META_CLI", "-o", out, *graph(trees[tree]), *common, *extra, cwd=trees[tree])
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        runs[name] = (tool_files(out, S.TILE_FILES), r.stdout)
    assert runs["first"][0] == runs["want"][0] and len(runs["want"][0]["tiles.txt"].splitlines()) > 3
    assert runs["first"][1].count("Collapsed repeated sites: ") == 4 and " disagreeing (first)\n" in runs["first"][1]


def test_metaprofile_tiles_dedup_with_contexts_collapses_once_and_splits(tmp_path, trees):
    common = ["--tiles", "500", "--iterations", "12", "--seed", "99", "--name", "dedup", "--contexts", "CG,CHG"]
    graph = lambda root: ["--methylome", root / "data" / "methylome", "--nodes", root / "data" / "nodelist.txt", "--edges",
                          root / "data" / "edgelist.txt"]
    runs = {}
    for name, tree, extra in (("want", "original", ["--sort"]), ("first", "doubled in order", ["--dedup", "first"])):
        out = tmp_path / name
        out.mkdir()
        r = S.run_tool("META_CLI", "-o", out, *graph(trees[tree]), *common, *extra, cwd=trees[tree])
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        runs[name] = {ctx: tool_files(out / ctx, S.TILE_FILES) for ctx in ("CG", "CHG")}
        assert r.stdout.count("Collapsed repeated sites: ") == (4 if name == "first" else 0)   # once per methylome, not per context
    assert runs["first"] == runs["want"] and runs["want"]["CG"]["raw.npy"] != runs["want"]["CHG"]["raw.npy"]


def test_dedup_flag_refusals(tmp_path):
    golden = ["-n", "./data/nodelist.txt", "-e", "./data/edgelist.txt", "-o", tmp_path]
    for extra in (["--dedup", "best", "--sites", "host"], ["--dedup", "best"],
                  ["--dedup", "best", "--sites", "device", "--parse", "host"]):
        r = S.run_tool("CLI", *golden, *extra, cwd=GOLDEN, timeout=60)
        assert r.returncode == 2 and "--dedup needs --sites device" in r.stderr, (extra, r.stderr)
    r = S.run_tool("CLI", *golden, "--sites", "device", "--dedup", "newest", cwd=GOLDEN, timeout=60)
    assert r.returncode == 2 and "--dedup expects one of first, last, best, drop" in r.stderr, r.stderr
    ped = tmp_path.parent / "pedigree_for_dedup.txt"
    ped.write_text("0 1 2 0.1\n")
    r = S.run_tool("CLI", "--pedigree", ped, "--p0uu", "0.5", "-o", tmp_path, "--sites", "device", "--dedup", "best", cwd=GOLDEN,
                   timeout=60)
    assert r.returncode == 2 and "--dedup" in r.stderr, r.stderr
    meth = GOLDEN / "data" / "methylome"
    tiles = ["-o", tmp_path, "--methylome", meth, "--nodes", GOLDEN / "data" / "nodelist.txt", "--edges",
             GOLDEN / "data" / "edgelist.txt"]
    for args, words in (([*tiles, "--tiles", "50000", "--dedup", "best", "--sites", "host"], "--sites host do not apply"),
                        ([*tiles, "--tiles", "50000", "--dedup", "best", "--parse", "host"], "--parse host"),
                        ([*tiles, "--tiles", "50000", "--dedup", "newest"], "--dedup expects one of"),
                        (["-o", tmp_path, "--dedup", "best"], "not to window directories"),
                        ([*tiles, "--genome", GOLDEN / "annotation.txt", "--dedup", "best"], "needs --sites device")):
        r = S.run_tool("META_CLI", *args, cwd=GOLDEN, timeout=60)
        assert r.returncode == 2 and words in r.stderr, (args, r.stderr)
    assert not any(tmp_path.iterdir())
    for tool in ("CLI", "META_CLI"):
        assert "--dedup" in S.run_tool(tool, "--help", timeout=60).stdout
