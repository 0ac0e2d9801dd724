"""abn_pairwise_transitions*: the 3 x 3 state transition table of every sample pair (the joint table behind DMatrix::from,
src/pedigree.rs:236-257) on the device, against the numpy model of tests/_transitions_model.py and — folded to `both` and
`diff` — against the existing divergence kernels on the same call.  Every comparison is exact integer equality."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import _tiles_model as T
import _transitions_model as M

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden"
PACKED_CHUNK_SITES = 32768   # kPmxWinPackedChunkSites (csrc/abn_packed_mask.hpp): longer windows are cut into chunks
MAX_JOBS = 2048              # kTransMaxJobs (csrc/abn_pairwise_transitions.hpp): (window, super-pair, chunk) units per launch
INVALID = 1                  # ABN_ERR_INVALID_ARG
FLT = 0.99
STATES = np.array([0, 1, 2, 0x80], dtype=np.uint8)


def _pair(n, a, b):
    return a * n - a * (a + 1) // 2 + (b - a - 1)


def _assert_folds(table, diff, both):
    tb, td = M.folds(table)
    assert np.array_equal(tb, both) and np.array_equal(td, diff)


@pytest.mark.parametrize("n", [2, 17, 65, 130])
def test_edge_windows_and_the_whole_matrix(abn, gpu_ctx, n):
    _, _, codes = M.random_codes(n, n, M.SITES)
    packed = abn.pack_codes(codes)
    begin, end = M.edge_windows()
    got = gpu_ctx.pairwise_transitions_windows_packed(packed, M.SITES, begin, end)
    assert got.dtype == np.uint64 and got.shape == (len(begin), n * (n - 1) // 2, 3, 3)
    want = (M.windows_table if n <= 17 else M.windows_table_by_planes)(codes, begin, end)
    for w in range(len(begin)):
        assert np.array_equal(got[w], want[w]), (w, begin[w], end[w])
    for w in np.flatnonzero(begin == end):
        assert not got[w].any()
    diff, both, _ = gpu_ctx.pairwise_divergence_windows_packed(packed, M.SITES, begin, end)
    _assert_folds(got, diff, both)
    whole = gpu_ctx.pairwise_transitions_packed(packed, M.SITES)
    assert whole.dtype == np.uint64 and np.array_equal(whole, (M.table if n <= 17 else M.table_by_planes)(codes))
    diff, both, _ = gpu_ctx.pairwise_divergence_packed(packed, M.SITES)
    _assert_folds(whole, diff, both)


def test_orientation_on_every_kind_of_tile(abn, gpu_ctx):
    """All 4 x 4 combinations of U / I / M / filtered in sixteen different odd counts, planted on (3, 9) — one 16-block —
    (3, 40) — two blocks of one group — and (3, 141) — two groups — at once; the planted columns straddle a super-step
    boundary, one window's begin and another's end.  A transposed tile or a swapped plane is a wrong count."""
    n, sites = 150, 1400
    rng = np.random.default_rng(7)
    codes = STATES[rng.integers(0, 4, size=(n, sites))]
    a, others = 3, (9, 40, 141)
    cols, counts = [], {}
    for ia in range(4):
        for ib in range(4):
            counts[(ia, ib)] = 2 * (4 * ia + ib) + 1                      # 1, 3, ..., 31
            cols += [(STATES[ia], STATES[ib])] * counts[(ia, ib)]
    assert sorted(counts.values()) == list(range(1, 32, 2))
    cols = np.array(cols, dtype=np.uint8)[rng.permutation(len(cols))]
    at = 301
    assert at // 256 != (at + len(cols) - 1) // 256
    codes[a, at: at + len(cols)] = cols[:, 0]
    for b in others:
        codes[b, at: at + len(cols)] = cols[:, 1]
    mid = at + len(cols) // 2 + 1
    begin = np.array([at + 7, 13, at, at - 3, mid, at + 1], dtype=np.int64)
    end = np.array([at + len(cols) + 50, mid, at + len(cols), at + len(cols) - 2, sites, at + 2], dtype=np.int64)
    got = gpu_ctx.pairwise_transitions_windows_packed(abn.pack_codes(codes), sites, begin, end)
    by_hand = np.array([[counts[(x, y)] for y in range(3)] for x in range(3)], dtype=np.uint64)
    assert by_hand[0, 2] != by_hand[2, 0] and by_hand[0, 1] != by_hand[1, 0]
    for b in others:
        assert np.array_equal(got[2][_pair(n, a, b)], by_hand), b      # window 2 is exactly the planted columns
    assert np.array_equal(got, M.windows_table_by_planes(codes, begin, end))


def test_outside_does_not_count(abn, gpu_ctx):
    n, sites = 21, 3001
    rng = np.random.default_rng(21)
    codes = STATES[rng.integers(0, 4, size=(n, sites))]
    begin = np.array([5, 100, 250, 300, 700, 1029, 1500, 2303, 2990], dtype=np.int64)
    end = np.array([6, 131, 263, 600, 1023, 1030, 2049, 2817, 2999], dtype=np.int64)
    inside = np.zeros(sites, dtype=bool)
    for b, e in zip(begin, end):
        inside[b:e] = True
    other = codes.copy()
    other[:, ~inside] = STATES[(np.searchsorted(STATES, codes[:, ~inside]) + rng.integers(1, 4, size=(n, (~inside).sum()))) % 4]
    assert np.all(other[:, ~inside] != codes[:, ~inside]) and np.array_equal(other[:, inside], codes[:, inside])
    ga = gpu_ctx.pairwise_transitions_windows_packed(abn.pack_codes(codes), sites, begin, end)
    gb = gpu_ctx.pairwise_transitions_windows_packed(abn.pack_codes(other), sites, begin, end)
    assert np.array_equal(ga, gb) and ga.max() > 0
    assert np.array_equal(ga, M.windows_table_by_planes(codes, begin, end))


def test_a_chunked_window_among_short_ones(abn, gpu_ctx):
    n, long_len, sites = 9, 200_003, 220_001
    assert long_len > 6 * PACKED_CHUNK_SITES             # several partial rows and the reduce kernel; the others are direct
    rng = np.random.default_rng(11)
    lens = rng.integers(50, 5001, size=11)
    _, _, codes = M.random_codes(12, n, sites)
    short_b = rng.integers(0, sites - 5000, size=11)
    begin = np.concatenate([short_b[:6], [9_999], short_b[6:]]).astype(np.int64)
    end = np.concatenate([short_b[:6] + lens[:6], [9_999 + long_len], short_b[6:] + lens[6:]]).astype(np.int64)
    packed = abn.pack_codes(codes)
    got = gpu_ctx.pairwise_transitions_windows_packed(packed, sites, begin, end)
    assert np.array_equal(got, M.windows_table_by_planes(codes, begin, end))
    # ... and the whole matrix, which is one chunked window
    assert np.array_equal(gpu_ctx.pairwise_transitions_packed(packed, sites), M.table_by_planes(codes))


def test_more_jobs_than_one_launch_holds(abn, gpu_ctx):
    """n = 65: two diagonal super-pairs and one off-diagonal per window — 2100 windows are 4200 and 2100 units"""
    n, W = 65, 2100
    sites = 4 * W + 41
    assert W > MAX_JOBS
    _, _, codes = M.random_codes(65, n, sites)
    begin = (4 * np.arange(W) + np.arange(W) % 3).astype(np.int64)
    end = begin + 40
    got = gpu_ctx.pairwise_transitions_windows_packed(abn.pack_codes(codes), sites, begin, end)
    assert np.array_equal(got, M.windows_table_by_planes(codes, begin, end))


def test_device_resident_entries(abn, gpu_ctx):
    """Packed codes and tables stay in HBM (buffers from the HIP runtime the product library already holds); a pointer 8
    bytes off the 16-byte alignment is refused."""
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
    hip.hipFree.argtypes = [C.c_void_p]
    n, sites = 21, 50_001
    _, _, codes = M.random_codes(4, n, sites)
    packed = abn.pack_codes(codes)
    stride = packed.shape[1]
    rng = np.random.default_rng(4)
    W = 12
    begin = rng.integers(0, sites - 40_000, size=W).astype(np.int64)
    lens = rng.integers(0, 40_000, size=W)
    lens[0], begin[1], lens[1] = 0, sites - 9000, 9000        # an empty window; one to the last site of the last row
    assert lens.max() > PACKED_CHUNK_SITES > lens.min()
    end = begin + lens
    npairs = n * (n - 1) // 2
    want = gpu_ctx.pairwise_transitions_windows_packed(packed, sites, begin, end)
    want_whole = gpu_ctx.pairwise_transitions_packed(packed, sites)
    assert np.array_equal(want, M.windows_table_by_planes(codes, begin, end))
    bufs = [C.c_void_p() for _ in range(2)]
    nbytes = 8 * 9 * W * npairs
    for ptr, size in zip(bufs, (packed.nbytes + 64, nbytes)):
        assert hip.hipMalloc(C.byref(ptr), size) == 0
    try:
        assert bufs[0].value % 16 == 0
        assert hip.hipMemcpy(bufs[0], packed.ctypes.data, packed.nbytes, 1) == 0
        assert hip.hipMemset(bufs[1], 7, nbytes) == 0
        ms = gpu_ctx.pairwise_transitions_windows_packed_dev(bufs[0].value, n, sites, stride, begin, end, bufs[1].value)
        assert ms > 0
        host = np.zeros(want.shape, dtype=np.uint64)
        assert hip.hipMemcpy(host.ctypes.data, bufs[1], nbytes, 2) == 0
        assert np.array_equal(host, want)
        assert hip.hipMemset(bufs[1], 7, nbytes) == 0
        ms = gpu_ctx.pairwise_transitions_packed_dev(bufs[0].value, n, sites, stride, bufs[1].value)
        assert ms > 0
        host = np.zeros((W,) + want_whole.shape, dtype=np.uint64)
        assert hip.hipMemcpy(host.ctypes.data, bufs[1], nbytes, 2) == 0
        assert np.array_equal(host[0], want_whole) and np.all(host[1:].view(np.uint8) == 7)
        for call in (lambda: gpu_ctx.pairwise_transitions_windows_packed_dev(bufs[0].value + 8, n, sites, stride, begin, end,
                                                                             bufs[1].value),
                     lambda: gpu_ctx.pairwise_transitions_packed_dev(bufs[0].value + 8, n, sites, stride, bufs[1].value)):
            with pytest.raises(abn.AbnError) as err:
                call()
            assert err.value.status == INVALID
        assert hip.hipMemcpy(host.ctypes.data, bufs[1], nbytes, 2) == 0
        assert np.array_equal(host[0], want_whole) and np.all(host[1:].view(np.uint8) == 7)     # nothing written
    finally:
        for ptr in bufs:
            hip.hipFree(ptr)


def test_arguments(abn, gpu_ctx):
    """the refusals of tests/test_pairwise_windows_packed.py::test_packed_windows_arguments, the output untouched"""
    sites = 300
    packed = abn.pack_codes(np.zeros((3, sites), dtype=np.uint8))
    assert packed.shape == (3, 128)
    for b, e in (([5], [4]), ([0], [sites + 1]), ([-1], [10]), ([0, 50], [10, 49]), ([0], [512])):
        with pytest.raises(abn.AbnError) as err:
            gpu_ctx.pairwise_transitions_windows_packed(packed, sites, b, e)
        assert err.value.status == INVALID
    i64p, u8p, u64p = C.POINTER(C.c_int64), C.POINTER(C.c_uint8), C.POINTER(C.c_uint64)
    zero, ten = np.zeros(1, dtype=np.int64), np.full(1, 10, dtype=np.int64)
    out = np.full(40, 7, dtype=np.uint64)
    fn, whole = gpu_ctx._L.abn_pairwise_transitions_windows_packed, gpu_ctx._L.abn_pairwise_transitions_packed

    def call(p=packed.ctypes.data_as(u8p), n=3, L=sites, stride=128, b=zero.ctypes.data_as(i64p),
             e=ten.ctypes.data_as(i64p), W=1):
        return fn(gpu_ctx._h, p, n, L, stride, b, e, W, out.ctypes.data_as(u64p))

    def call_whole(p=packed.ctypes.data_as(u8p), n=3, L=sites, stride=128):
        return whole(gpu_ctx._h, p, n, L, stride, out.ctypes.data_as(u64p))

    assert call() == 0 and out[:27].reshape(3, 9)[:, 0].tolist() == [10, 10, 10] and out[:27].sum() == 30
    assert np.all(out[27:] == 7)
    out[:] = 7
    assert call_whole() == 0 and out[:27].reshape(3, 9)[:, 0].tolist() == [sites] * 3 and np.all(out[27:] == 7)
    out[:] = 7
    for f in (call, call_whole):        # what the one-matrix packed entry refuses
        assert f(p=None) == INVALID and f(n=0) == INVALID and f(n=-2) == INVALID and f(L=-1) == INVALID
        assert f(stride=96) == INVALID and f(stride=64) == INVALID and f(stride=-64) == INVALID
        assert f(n=65536) == INVALID
    assert call(W=-1) == INVALID and call(b=None) == INVALID and call(e=None) == INVALID
    huge = np.full(1, 8192 << 30, dtype=np.int64)    # a chunk of the window would reach 2^30 sites
    assert call(L=int(huge[0]), stride=int(huge[0]) // 4, e=huge.ctypes.data_as(i64p)) == INVALID
    assert np.all(out == 7)
    assert call(W=0) == 0 and call(W=0, b=None, e=None) == 0 and call(n=1) == 0 and call_whole(n=1) == 0
    assert np.all(out == 7)
    assert gpu_ctx.pairwise_transitions_windows_packed(packed, sites, [], []).shape == (0, 3, 3, 3)
    assert gpu_ctx.pairwise_transitions_windows_packed(packed[:1], sites, [0, 10], [10, 20]).shape == (2, 0, 3, 3)
    assert gpu_ctx.pairwise_transitions_packed(packed[:1], sites).shape == (0, 3, 3)
    empty = gpu_ctx.pairwise_transitions_packed(abn.pack_codes(np.zeros((3, 0), dtype=np.uint8)), 0)
    assert empty.shape == (3, 3, 3) and not empty.any()


# ---------------------------------------------------------------- the handles, on the golden methylomes
def _golden_samples(drop, sort=False):
    """the four golden methylomes, sample s without the CG lines drop[s] (indices among its CG lines: the context that
    is read); sort: the lines by chromosome, start and strand, one run order for all (the files' own differ) -> (texts,
    per sample [(key, byte code)] in line order)"""
    texts, parsed = [], []
    for s, path in enumerate(sorted((GOLDEN / "data" / "methylome").glob("*.txt"))):
        lines = path.read_text().splitlines()
        key = lambda f: (T.chromosome_key(f[0]), int(f[1]), T.STRAND[f[2]])
        cg = [k for k, ln in enumerate(lines[1:]) if ln.split("\t")[3] == "CG"]
        gone = {cg[k] for k in drop[s]}
        body = [ln for k, ln in enumerate(lines[1:]) if k not in gone]
        if sort:
            body.sort(key=lambda ln: key(ln.split("\t")))
        texts.append(("\n".join([lines[0]] + body) + "\n").encode())
        fields = [ln.split("\t") for ln in body]
        parsed.append([(key(f), "UIM".index(f[7]) | (0x80 if float(f[6]) < FLT else 0)) for f in fields if f[3] == "CG"])
    return texts, parsed


def _columns(parsed, align):
    """the aligned byte codes (n, columns) and the columns' keys.  none: line k of every sample is column k, its key sample
    0's; union: the sorted keys any sample holds, 0x80 where a sample lacks one"""
    if align == "none":
        assert len({len(p) for p in parsed}) == 1
        return np.array([[c for _, c in p] for p in parsed], dtype=np.uint8), [k for k, _ in parsed[0]]
    held = [dict(p) for p in parsed]
    keys = sorted(set.union(*[set(h) for h in held]))
    return np.array([[h.get(k, 0x80) for k in keys] for h in held], dtype=np.uint8), keys


@pytest.fixture(scope="module")
def golden(abn, gpu_ctx):
    from test_tiles_gpu import resident
    import _parse_model as P

    L = P.hostlib()
    made = {}
    for align in ("none", "union"):
        drop = [set()] * 4 if align == "none" else [set(range(10 + 7 * s, 500, 41 + 3 * s)) for s in range(4)]
        texts, parsed = _golden_samples(drop, sort=align == "union")
        sites = [resident(gpu_ctx, L, t) for t in texts]
        made[align] = {"sites": sites, "parsed": parsed,
                       "codes": abn.Codes.from_parsed(gpu_ctx, sites, posterior_max_filter=FLT, align=align),
                       "tiles": abn.Tiles.from_parsed(gpu_ctx, sites, posterior_max_filter=FLT, align=align)}
    yield made
    for m in made.values():
        m["codes"].close(), m["tiles"].close()
        for s in m["sites"]:
            s.close()


@pytest.mark.parametrize("align", ["none", "union"])
def test_codes_and_tiles_handles(abn, gpu_ctx, golden, align):
    h = golden[align]
    codes, keys = _columns(h["parsed"], align)
    assert len(keys) == 500
    if align == "union":
        assert sum(len(p) for p in h["parsed"]) < 4 * 500 and codes.shape[1] == 500          # placeholders, in no entry
    got = h["codes"].transitions()
    assert got.dtype == np.uint64 and got.shape == (6, 3, 3) and np.array_equal(got, M.table(codes))
    diff, both, _ = h["codes"].pairwise()
    _assert_folds(got, diff, both)
    # tiles: bins of 250 bp over chromosome 2 (starts: -1 on the other chromosomes)
    two = T.chromosome_key("2")
    starts = np.array([k[1] if k[0] == two else -1 for k in keys], dtype=np.int64)
    assert (starts >= 0).sum() > 100
    lo = np.arange(0, int(starts.max()) + 250, 250, dtype=np.int64)
    assert len(lo) >= 6
    tiles = h["tiles"]
    chrom = np.full(len(lo), two, dtype=np.int32)
    tiles.set_intervals(chrom, lo, lo + 250)
    got = tiles.transitions()
    assert got.dtype == np.uint64 and got.shape == (len(lo), 6, 3, 3)
    for t, b in enumerate(lo):
        sel = (starts >= b) & (starts < b + 250)
        assert np.array_equal(got[t], M.table(codes[:, sel])), t
    diff, both, _ = tiles.pairwise()
    _assert_folds(got, diff, both)
    # one pooled region list: pool 0 = bins 0, 2, 4 (and 2 once more), pool 1 = bin 1, pool 2 = nothing
    ip = np.array([0, 1, 0, 0, 0], dtype=np.int32)
    at = np.array([0, 1, 2, 4, 2])
    tiles.set_pools(chrom[:5], lo[at], lo[at] + 250, ip, 3)
    try:
        got = tiles.transitions()
        assert got.shape == (3, 6, 3, 3) and not got[2].any()
        in_bin = lambda k: (starts >= lo[k]) & (starts < lo[k] + 250)
        assert np.array_equal(got[0], M.table(codes[:, in_bin(0) | in_bin(2) | in_bin(4)]))
        assert np.array_equal(got[1], M.table(codes[:, in_bin(1)]))
        diff, both, _ = tiles.pairwise()
        _assert_folds(got, diff, both)
    finally:
        tiles.set_intervals(chrom, lo, lo + 250)


# ---------------------------------------------------------------- the tools
def _run(tool, *args, cwd=None):
    from alphabeta_rs_amd import build as B

    B.build_host()
    r = subprocess.run([str(getattr(B, tool)), *map(str, args)], capture_output=True, text=True, timeout=300, cwd=cwd)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r


def _files(out):
    return {str(p.relative_to(out)): p.read_bytes() for p in sorted(out.rglob("*")) if p.is_file()}


NODES = [("0_0", 0), ("1_2", 1), ("4_2", 4), ("4_8", 4)]          # the rows of the bundled nodelist with meth = Y
PAIR_LINES = [f"{a[0]}\t{b[0]}\t{a[1]}\t{b[1]}" for i, a in enumerate(NODES) for b in NODES[i + 1:]]


@pytest.mark.parametrize("sites", ["host", "device"])
def test_alphabeta_transitions_on_the_bundled_data(tmp_path, sites):
    common = ["-i", "20", "--seed", "4711", "-n", "./data/nodelist.txt", "-e", "./data/edgelist.txt", "--sites", sites]
    plain, flagged = tmp_path / "plain", tmp_path / "flagged"
    plain.mkdir(), flagged.mkdir()
    _run("CLI", *common, "-o", plain, cwd=GOLDEN)
    _run("CLI", *common, "-o", flagged, "--transitions", cwd=GOLDEN)
    a, b = _files(plain), _files(flagged)
    assert "transitions.txt" not in a and set(b) == set(a) | {"transitions.txt"}
    for name in a:
        assert a[name] == b[name], name                                   # every other file: not a byte changes
    lines = b["transitions.txt"].decode().splitlines()
    assert lines[0].split("\t") == ["sample_a", "sample_b", "generation_a", "generation_b",
                                    "UU", "UI", "UM", "IU", "II", "IM", "MU", "MI", "MM"]
    assert ["\t".join(ln.split("\t")[:4]) for ln in lines[1:]] == PAIR_LINES
    got = np.array([[int(x) for x in ln.split("\t")[4:]] for ln in lines[1:]], dtype=np.uint64).reshape(6, 3, 3)
    _, parsed = _golden_samples([set()] * 4)
    codes, _ = _columns(parsed, "none")
    assert np.array_equal(got, M.table(codes)) and got.sum() > 0


def test_metaprofile_transitions_in_one_and_two_contexts(abn, gpu_ctx, tmp_path):
    graph = ["--methylome", GOLDEN / "data" / "methylome", "--nodes", GOLDEN / "data" / "nodelist.txt", "--edges",
             GOLDEN / "data" / "edgelist.txt", "--tiles", "50000", "--iterations", "12", "--seed", "99", "--name", "t"]
    runs = {}
    for name, extra in (("plain", []), ("CG", ["--transitions"]), ("CHH", ["--transitions", "--contexts", "CHH"]),
                        ("both", ["--transitions", "--contexts", "CG,CHH"])):
        out = tmp_path / name
        out.mkdir()
        _run("META_CLI", "-o", out, *graph, *extra, cwd=GOLDEN)
        runs[name] = _files(out)
    new = {"transitions.npy", "transition_pairs.txt"}
    assert set(runs["CG"]) == set(runs["plain"]) | new and not new & set(runs["plain"])
    for name in runs["plain"]:
        assert runs["plain"][name] == runs["CG"][name], name
    assert set(runs["both"]) == {f"{c}/{f}" for c in ("CG", "CHH") for f in runs["CG"]}
    for c in ("CG", "CHH"):
        for f in runs[c]:
            assert runs["both"][f"{c}/{f}"] == runs[c][f], (c, f)         # the single-context run's files, byte for byte
    assert runs["CG"]["transitions.npy"] != runs["CHH"]["transitions.npy"]
    assert runs["CG"]["transition_pairs.txt"].decode().splitlines() == PAIR_LINES
    # against the handle on the same methylomes and tiles
    from test_tiles_gpu import resident
    import _parse_model as P

    L = P.hostlib()
    texts, _ = _golden_samples([set()] * 4)
    samples = [resident(gpu_ctx, L, t) for t in texts]
    tiles = abn.Tiles.from_parsed(gpu_ctx, samples, posterior_max_filter=FLT)
    try:
        tiles.set_fixed(50000)
        want = tiles.transitions()
        got = np.load(tmp_path / "CG" / "transitions.npy")
        n_tiles = len(runs["CG"]["tiles.txt"].decode().splitlines()) - 1
        assert got.dtype == np.dtype("<u8") and got.flags["C_CONTIGUOUS"] and got.shape == (n_tiles, 6, 9)
        assert np.array_equal(got, want.reshape(n_tiles, 6, 9)) and got.sum() > 0
    finally:
        tiles.close()
        for s in samples:
            s.close()


def test_transitions_flag_is_refused_where_it_does_not_apply(tmp_path):
    from alphabeta_rs_amd import build as B

    B.build_host()
    graph = ["--methylome", GOLDEN / "data" / "methylome", "--nodes", GOLDEN / "data" / "nodelist.txt", "--edges",
             GOLDEN / "data" / "edgelist.txt"]
    for args in (["-o", tmp_path, "--transitions"], ["-o", tmp_path, *graph, "--genome", GOLDEN / "annotation.txt", "--transitions"]):
        r = subprocess.run([str(B.META_CLI), *map(str, args)], capture_output=True, text=True, timeout=60, cwd=str(GOLDEN))
        assert r.returncode == 2 and "--transitions belongs to --tiles and --regions" in r.stderr
    assert not list(tmp_path.iterdir())
