"""Region-level states on the device (abn_packed_region_states*, abn_tiles_region_states, abn_regions_*;
alphabeta_rs_amd/csrc/abn_regions.hpp) against the numpy model of tests/_regions_model.py bit for bit: the fused kernel on
thousands of short tiles, on the edge cuts, on empty, overlapping and long windows (the census route), under a permuting
and repeating column map; the identity law; the region matrix of a tiles handle with its groups, census, scan and
transition tables; the refusals; and `metaprofile_alphabeta --region-states`."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import _regions_model as R
import _sim_model as S
import _tile_pools_model as PM
import _tiles_model as T
import _windows_model as M
from test_tiles_gpu import (ALIGNS, FLT, INVALID, N, NAMES, L, graph_files, handles, inputs, run_cli)  # noqa: F401

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def G():
    from alphabeta_rs_amd import regions

    return regions


@pytest.fixture(scope="module")
def hip():
    h = C.CDLL("libamdhip64.so")        # the HIP runtime the product library already holds
    h.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    h.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    h.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
    h.hipFree.argtypes = [C.c_void_p]
    return h


RULE = (1, 2, 3, 2)            # lo, hi, den, min_kept
SITES = 70_000


@pytest.fixture(scope="module")
def big():
    """n = 3, L = 70 000, random fields including 3; about 5 000 contiguous tiles of 1..40 sites (a new pass over the row from
    another offset when one ends), the cuts of the CPU tier, empty and overlapping windows, long windows of 5 000 and of
    40 000 sites — the latter across the census's chunk cut at 32 768 — and the model's answer, made once"""
    rng = np.random.default_rng(20260102)
    fields = R.random_fields(rng, 3, SITES)
    b, e, at, offset = [], [], 0, 0
    while len(b) < 5000:
        length = int(rng.integers(1, 41))
        if at + length > SITES:
            offset += 7
            at = offset
        b.append(at), e.append(at + length)
        at += length
    cuts = (0, 1, 15, 16, 17, 255, 256, 257, SITES)
    for lo in cuts:
        for hi in cuts:
            if lo <= hi:
                b.append(lo), e.append(hi)
    b += [SITES, 33_000, 100, 110, 1_234, 20_001, 3]                # empty twice, two overlapping, the long ones
    e += [SITES, 33_000, 130, 140, 6_234, 60_001, 3 + 64]
    b, e = np.array(b, dtype=np.int64), np.array(e, dtype=np.int64)
    if len(b) % 16 == 0:
        b, e = np.append(b, 5), np.append(e, 9)
    length = (e - b).tolist()
    assert 5_000 in length and 40_000 in length and 64 in length and 0 in length and len(b) % 16 != 0 and len(b) > 16 * 256
    assert 20_001 // 256 * 256 + 32_768 < 60_001                   # the chunk cut lies inside the 40 000-site window
    src = np.concatenate((rng.permutation(len(b)), rng.integers(0, len(b), size=777))).astype(np.int32)
    packed = S.pack(fields)
    return {"fields": fields, "packed": packed, "b": b, "e": e, "src": src,
            "want": R.region_states(packed, SITES, b, e, RULE), "want_src": R.region_states(packed, SITES, b, e, RULE, src)}


@pytest.mark.parametrize("long_sites", (0, 64))
def test_region_states_equal_the_model(G, gpu_ctx, big, long_sites):
    got = G.region_states(gpu_ctx, big["packed"], SITES, big["b"], big["e"], *RULE, long_sites=long_sites)
    assert got.dtype == np.uint8 and got.shape == big["want"].shape and got.tobytes() == big["want"].tobytes()
    assert set(np.unique(R.unpack(got, len(big["b"]))).tolist()) == {0, 1, 2, 3}


def test_region_states_under_a_permuting_and_repeating_column_map(G, gpu_ctx, big):
    got = G.region_states(gpu_ctx, big["packed"], SITES, big["b"], big["e"], *RULE, src=big["src"])
    assert got.shape == big["want_src"].shape and got.tobytes() == big["want_src"].tobytes()
    host = G.region_states_host(big["packed"], SITES, big["b"], big["e"], *RULE, src=big["src"], walk=True)
    assert host.tobytes() == got.tobytes()


def test_device_entry_gives_the_same_bytes_and_two_times(G, abn, gpu_ctx, hip, big):
    packed, want = big["packed"], big["want_src"]
    bufs = [C.c_void_p(), C.c_void_p()]
    assert hip.hipMalloc(C.byref(bufs[0]), packed.nbytes) == 0 and hip.hipMalloc(C.byref(bufs[1]), want.nbytes) == 0
    try:
        assert hip.hipMemcpy(bufs[0], packed.ctypes.data, packed.nbytes, 1) == 0
        for long_sites in (0, 64):
            assert hip.hipMemset(bufs[1], 0x5A, want.nbytes) == 0
            ms = G.region_states_dev(gpu_ctx, bufs[0].value, 3, SITES, packed.shape[1], big["b"], big["e"], *RULE, bufs[1].value,
                                     src=big["src"], long_sites=long_sites)
            assert ms.shape == (2,) and np.isfinite(ms).all() and (ms > 0).all()      # the long windows' census, the kernel
            got = np.zeros_like(want)
            assert hip.hipMemcpy(got.ctypes.data, bufs[1], got.nbytes, 2) == 0
            assert got.tobytes() == want.tobytes()
        args = dict(packed_ptr=bufs[0].value, n_samples=3, n_sites=SITES, row_stride=packed.shape[1], begin=big["b"], end=big["e"],
                    lo_num=1, hi_num=2, den=3, min_kept=2, out_ptr=bufs[1].value)
        for words, change in (("16-byte aligned", dict(packed_ptr=bufs[0].value + 8)), ("row_stride_bytes", dict(row_stride=64)),
                              ("is not a column range", dict(n_sites=SITES - 1)), ("null/size", dict(out_ptr=0)),
                              ("lo_num <= hi_num <= den", dict(hi_num=4)), ("min_kept", dict(min_kept=0)),
                              ("long_sites", dict(long_sites=24)), ("column 2", dict(src=[0, 1, len(big["b"])])),
                              ("n_columns is not n_windows", dict(n_columns=3))):
            with pytest.raises(abn.AbnError) as err:
                G.region_states_dev(gpu_ctx, **{**args, **change})
            assert err.value.status == INVALID and words in str(err.value), str(err.value)
        assert G.region_states_dev(gpu_ctx, **{**args, "src": np.zeros(0, dtype=np.int32)}).tolist() == [0.0, 0.0]   # C = 0
    finally:
        for ptr in bufs:
            hip.hipFree(ptr)


@pytest.mark.parametrize("n", (1, 65))
def test_rows_on_the_grid_and_a_ragged_last_dword(G, gpu_ctx, n):
    """L = 1 000: the last source dword holds 8 sites; n = 65: the grid's second dimension"""
    rng = np.random.default_rng(40 + n)
    sites = 1_000
    fields = R.random_fields(rng, n, sites)
    packed = S.pack(fields)
    b = np.concatenate((np.arange(0, sites, 3), [0, 990, 992, 999, 1000, 0])).astype(np.int64)
    e = np.concatenate((np.minimum(np.arange(0, sites, 3) + 3, sites), [1000, 1000, 1000, 1000, 1000, 500])).astype(np.int64)
    for long_sites in (0, 64):
        got = G.region_states(gpu_ctx, packed, sites, b, e, 1, 3, 4, 1, long_sites=long_sites)
        assert got.tobytes() == R.region_states(packed, sites, b, e, (1, 3, 4, 1)).tobytes()


def test_identity_law(G, gpu_ctx):
    """every window one site under (1, 3, 4), min_kept 1: the levels 0, 1/2, 1 call 0, 1, 2, a filtered site calls 3 — the
    region matrix is the source matrix, and its scan the source's"""
    rng = np.random.default_rng(9)
    sites = 1_000
    packed = S.pack(R.random_fields(rng, 3, sites))
    b = np.arange(sites, dtype=np.int64)
    got = G.region_states(gpu_ctx, packed, sites, b, b + 1, 1, 3, 4, 1)
    assert got.shape == packed.shape and got.tobytes() == packed.tobytes()
    for x, y in zip(gpu_ctx.pairwise_divergence_packed(got, sites), gpu_ctx.pairwise_divergence_packed(packed, sites)):
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes()


# ---------------------------------------------------------------- the region matrix of a tiles handle
def everything(reg):
    return (reg.packed(), reg.order(), *reg.layout(), reg.census(), *reg.pairwise(), reg.transitions())


def assert_regions_equal_model(reg, fields, begin, end, rule, group, n_groups):
    """matrix, order, layout, census, scan and tables of a Regions against the model over the tiles' column ranges"""
    T_ = len(begin)
    src, gb, ge = R.group_order(np.zeros(T_, dtype=np.int64) if group is None else group, n_groups)
    n, Cn = fields.shape[0], len(src)
    want = R.region_fields(fields, begin, end, rule, src)
    info = reg.info()
    assert info == {"n_samples": n, "n_columns": Cn, "row_stride": max(S.row_stride(Cn), 64), "n_groups": n_groups}
    order = reg.order()
    assert order.dtype == np.int32 and order.tolist() == src.tolist()
    lb, le = reg.layout()
    assert lb.dtype == le.dtype == np.int64 and lb.tolist() == gb.tolist() and le.tolist() == ge.tolist()
    packed = reg.packed()
    assert packed.tobytes() == S.pack(want, stride=info["row_stride"]).tobytes()
    census = reg.census()
    assert census.dtype == np.uint64 and census.shape == (n_groups, n, 3)
    assert np.array_equal(census.astype(np.int64), R.counts(want, gb, ge))
    diff, both, dval = reg.pairwise()
    wd, wb, wv = R.pairwise(want, gb, ge)
    assert diff.dtype == both.dtype == np.uint64 and np.array_equal(diff, wd) and np.array_equal(both, wb)
    assert np.array_equal(dval, wv, equal_nan=True) and np.array_equal(np.isnan(dval), both == 0)
    table = reg.transitions()
    assert table.dtype == np.uint64 and np.array_equal(table, R.pair_tables(want, gb, ge))
    ms = reg.kernel_ms()
    assert ms.shape == (2,) and np.isfinite(ms).all() and (ms[1] > 0 or Cn == 0)
    return want


@pytest.mark.parametrize("align", ALIGNS)
def test_regions_of_tiles_equal_the_model(abn, G, gpu_ctx, inputs, handles, align):
    rows, values, keeps = inputs
    h = handles[align]
    tiles, model = h["tiles"], h["model"]
    fields = np.stack([c["field"] for c in model[3]])
    explicit, names = T.tile_list(rows)
    called = set()
    for setter in ("intervals", "fixed"):
        if setter == "intervals":
            tiles.set_intervals(*explicit)
        else:
            tiles.set_fixed(1 << 20)                                           # thousands of tiles, most of them empty
        begin, end = tiles.layout()
        T_ = len(begin)
        assert (end - begin).max() > 16 and (end == begin).any()
        interleaved = (np.arange(T_) % 2).astype(np.int32)
        interleaved[::5] = -1
        with_empty = np.where(np.arange(T_) % 3 == 0, 0, 2).astype(np.int32)   # group 1 holds no tile
        for rule, group, n_groups in (((1, 3, 4, 1), None, 1), ((250_000, 750_000, 1_000_000, 2), interleaved, 2),
                                      ((1, 2, 3, 1), with_empty, 3), ((1, 3, 4, 1), np.full(T_, -1, dtype=np.int32), 1)):  # ... and no column at all
            reg = G.from_tiles(tiles, *rule, group=group, n_groups=n_groups)
            try:
                want = assert_regions_equal_model(reg, fields, begin, end, rule, group, n_groups)
                called |= set(np.unique(want).tolist())
                if group is with_empty:
                    assert reg.layout()[0][1] == reg.layout()[1][1] and not reg.census()[1].any() and np.isnan(reg.pairwise()[2][1]).all()
            finally:
                reg.close()
        if setter == "fixed":
            assert T_ > 2 * 256                                                # several workgroups per row
    assert called == {0, 1, 2, 3}


def test_regions_survive_the_tiles_handle_and_refusals_leave_it_working(abn, G, gpu_ctx, inputs, handles):
    rows, values, keeps = inputs
    h = handles["none"]
    fields = np.stack([c["field"] for c in h["model"][3]])
    tiles = abn.Tiles.from_parsed(gpu_ctx, h["sites"], posterior_max_filter=FLT, align="none")
    try:
        with pytest.raises(abn.AbnError) as err:                               # before any set_*
            G.from_tiles(tiles, 1, 3, 4)
        assert err.value.status == INVALID and "no tiles yet" in str(err.value)
        (ic, ilo, ihi, ip), names, _ = PM.pool_list(rows)
        tiles.set_pools(ic, ilo, ihi, ip, len(names))
        with pytest.raises(abn.AbnError) as err:                               # with pools set
            G.from_tiles(tiles, 1, 3, 4)
        assert err.value.status == INVALID and "a pool is a class of sites, not a region" in str(err.value)
        assert tiles.info()["n_tiles"] == len(names) and tiles.pairwise()[1].shape[0] == len(names)   # still pooled, still works
        tiles.set_fixed(1 << 20)
        T_ = tiles.info()["n_tiles"]
        for words, kw in (("lo_num <= hi_num <= den", dict(lo_num=3, hi_num=2, den=4)), ("min_kept", dict(min_kept=0)),
                          ("n_groups", dict(n_groups=0)), ("tile 1: group 2", dict(group=np.array([0, 2] + [0] * (T_ - 2)), n_groups=2)),
                          ("tile 0: group -2", dict(group=np.full(T_, -2)))):
            with pytest.raises(abn.AbnError) as err:
                G.from_tiles(tiles, **{**dict(lo_num=1, hi_num=3, den=4), **kw})
            assert err.value.status == INVALID and words in str(err.value), str(err.value)
        with pytest.raises(ValueError):
            G.from_tiles(tiles, 1, 3, 4, group=np.zeros(T_ + 1))
        begin, end = tiles.layout()
        reg = G.from_tiles(tiles, 1, 3, 4, 1)
        before = everything(reg)
        assert_regions_equal_model(reg, fields, begin, end, (1, 3, 4, 1), None, 1)
        tiles.set_fixed(1 << 28)                                               # the tiles change, the regions do not
        assert tiles.info()["n_tiles"] != T_
        for x, y in zip(everything(reg), before):
            assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()
        tiles.close()
        tiles = None
        for x, y in zip(everything(reg), before):                              # ... and outlive the handle
            assert x.tobytes() == y.tobytes()
        reg.close()
    finally:
        if tiles is not None:
            tiles.close()


# ---------------------------------------------------------------- metaprofile_alphabeta --region-states
N_SITES = 1200


def level_methylomes(meth: Path):
    """four methylomes of the bundled pedigree's sampled nodes: 1200 sites on chromosome 1 at 10 i + 5, every posterior above
    the filter, rc.meth.lvl = status / 2 (0, 0.5, 1), the later generations' statuses drifting from the founder's
    -> fields uint8 (4, 1200) in NAMES' order"""
    rng = np.random.default_rng(8)
    status = rng.choice([0, 2], size=N_SITES, p=[0.6, 0.4])
    fields = []
    meth.mkdir()
    for k, name in enumerate(NAMES):
        if k:
            status = np.where(rng.random(N_SITES) < 0.04 * k, rng.integers(0, 3, size=N_SITES), status)
        lines = [M.site_line("1", 10 * i + 5, "+-"[i % 2], "UIM"[int(s)], 0.9999, 0.5 * float(s)) for i, s in enumerate(status)]
        (meth / name).write_text(M.HEADER + "".join(l + "\n" for l in lines))
        fields.append(status.astype(np.uint8))
    return np.stack(fields)


def result_rows(path):
    """results.txt -> (header, [row fields])"""
    lines = path.read_text().splitlines()
    return lines[0].split(";"), [l.split(";") for l in lines[1:] if l]


def test_metaprofile_single_site_regions_equal_one_interval(tmp_path):
    """One single-site region per site under --region-states 0.25,0.75: the level 0, 1/2, 1 of the site calls its own status,
    so the one region-level pedigree is the site-level pedigree of ONE interval over everything — the same D, the same level
    folds, the same window index 0: raw.npy byte for byte and every results.txt column but `region`"""
    meth = tmp_path / "methylome"
    fields = level_methylomes(meth)
    graph_files(tmp_path, meth)
    (tmp_path / "sites.bed").write_text("".join(f"1\t{10 * i + 5}\t{10 * i + 6}\n" for i in range(N_SITES)))
    (tmp_path / "whole.bed").write_text(f"1\t0\t{10 * N_SITES + 5}\n")
    common = ["--methylome", meth, "--nodes", tmp_path / "nodelist.fn", "--edges", tmp_path / "edgelist.fn", "--iterations", "20",
              "--seed", "77"]
    a, b = tmp_path / "a", tmp_path / "b"
    a.mkdir(), b.mkdir()
    r1 = run_cli("-o", a, *common, "--regions", tmp_path / "sites.bed", "--region-states", "0.25,0.75")
    assert r1.returncode == 0, r1.stdout[-2000:] + r1.stderr[-2000:]
    r2 = run_cli("-o", b, *common, "--regions", tmp_path / "whole.bed")
    assert r2.returncode == 0, r2.stdout[-2000:] + r2.stderr[-2000:]
    assert (a / "raw.npy").read_bytes() == (b / "raw.npy").read_bytes() and np.load(a / "raw.npy").shape == (20, 7, 1)
    (h1, rows1), (h2, rows2) = result_rows(a / "results.txt"), result_rows(b / "results.txt")
    assert h1 == h2 and len(rows1) == len(rows2) == 1
    at = h1.index("region")
    assert rows1[0][:at] == rows2[0][:at] and rows1[0][at + 1:] == rows2[0][at + 1:] and rows1[0][at] == "regions"
    assert rows1[0][h1.index("window")] == "0" and rows1[0][h1.index("cg_count")] == str(N_SITES)
    states = np.load(a / "region_states.npy")
    assert states.dtype == np.uint8 and np.array_equal(states, fields)
    assert sorted(p.name for p in a.iterdir()) == ["raw.npy", "region_states.npy", "regions.txt", "results.txt"]
    listed = (a / "regions.txt").read_text().splitlines()
    assert listed[0] == "column;tile;chromosome;start;end;cg_count;group" and len(listed) == N_SITES + 1
    assert listed[1] == "0;0;1;5;6;1;0" and listed[-1] == f"{N_SITES - 1};{N_SITES - 1};1;{10 * N_SITES - 5};{10 * N_SITES - 4};1;0"


def test_metaprofile_region_pools_and_the_files_without_the_flag(tmp_path):
    """--pool with two names: the rows stay one region each, grouped by name — two rows of results.txt, groups.txt, and a
    region_states.npy equal to the model; without the flag a --tiles run writes exactly the files it wrote before"""
    meth = tmp_path / "methylome"
    fields = level_methylomes(meth)
    graph_files(tmp_path, meth)
    per = 4                                                                     # sites per row; rows alternate te / gene
    rows = [(40 * k, 40 * (k + 1), ("te", "gene")[k % 2]) for k in range(N_SITES // per)]
    text = "".join(f"1\t{lo}\t{hi}\t{name}\n" for lo, hi, name in rows[:7]) + "1\t0\t400\n" + \
        "".join(f"1\t{lo}\t{hi}\t{name}\n" for lo, hi, name in rows[7:]) + "1\t20\t100\tgene\n"     # unnamed: skipped; overlapping: fine
    (tmp_path / "rows.bed").write_text(text)
    common = ["--methylome", meth, "--nodes", tmp_path / "nodelist.fn", "--edges", tmp_path / "edgelist.fn", "--iterations", "20",
              "--seed", "77"]
    out = tmp_path / "out"
    out.mkdir()
    r = run_cli("-o", out, *common, "--regions", tmp_path / "rows.bed", "--pool", "--region-states", "0.3,0.7",
                "--region-min-sites", "2", "--transitions")
    assert r.returncode == 0 and "Skipped 1 regions without a name" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    begin = np.array([lo // 10 for lo, _, _ in rows] + [2], dtype=np.int64)      # site i at 10 i + 5
    end = np.array([hi // 10 for _, hi, _ in rows] + [10], dtype=np.int64)
    group = np.array([k % 2 for k in range(len(rows))] + [1])
    src, gb, ge = R.group_order(group, 2)
    want = R.region_fields(fields, begin, end, (300_000, 700_000, 1_000_000, 2), src)
    states = np.load(out / "region_states.npy")
    assert states.dtype == np.uint8 and states.shape == want.shape and np.array_equal(states, want)
    assert set(np.unique(want).tolist()) >= {0, 1, 2}
    header, res = result_rows(out / "results.txt")
    assert [x[header.index("window")] for x in res] == ["0", "1"] and [x[header.index("region")] for x in res] == ["te", "gene"]
    assert [x[header.index("cg_count")] for x in res] == [str(int(ge[0] - gb[0])), str(int(ge[1] - gb[1]))]
    assert (out / "groups.txt").read_text().splitlines() == ["group;name;regions;fitted", f"0;te;{ge[0] - gb[0]};1", f"1;gene;{ge[1] - gb[1]};1"]
    listed = [l.split(";") for l in (out / "regions.txt").read_text().splitlines()[1:]]
    assert [int(l[1]) for l in listed] == src.tolist() and [int(l[6]) for l in listed] == [0] * int(ge[0]) + [1] * int(ge[1] - gb[1])
    assert listed[-1][2:6] == ["1", "20", "100", "8"]
    assert np.load(out / "raw.npy").shape == (20, 7, 2)
    table = np.load(out / "transitions.npy")
    assert np.array_equal(table.reshape(2, -1, 3, 3), R.pair_tables(want, gb, ge))
    assert sorted(p.name for p in out.iterdir()) == ["groups.txt", "raw.npy", "region_states.npy", "regions.txt", "results.txt",
                                                     "transition_pairs.txt", "transitions.npy"]
    plain = tmp_path / "plain"
    plain.mkdir()
    r = run_cli("-o", plain, *common, "--tiles", "3000")
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert sorted(p.name for p in plain.iterdir()) == ["raw.npy", "results.txt", "tiles.txt"]
