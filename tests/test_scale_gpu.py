"""The resident methylome path past one scan workgroup's first trip: a slab of more than 1024 K1 blocks and more than
1024 K3 runs, a parent of more than 1024 split workgroups, chunks of more than 65 536 records, samples of more than 65 536
sites — the sizes at which abn_parse_scan_kernel and abn_common_scan_kernel walk a serial slice per lane and
abn_sites_flagged_kernel takes a second grid-stride trip.  The reference is the arrays the inputs were written from
(tests/_scale_model.py; tests/test_scale_cpu.py holds them against the host parsers and the serial forms), floats
compared as bytes.  Every test first asserts from its own input that the path it is there for is reached."""
import numpy as np
import pytest

import _codes_model as K
import _contexts_model as CX
import _parse_model as P
import _scale_model as S
import _tiles_model as T
import _transitions_model as TR

pytestmark = pytest.mark.gpu
FLT = K.FILTER
KEYS = [k for k, _ in P.FIELDS] + ["status_flag"]
TILE = 50000


@pytest.fixture(scope="module")
def L():
    return CX.hostlib()


@pytest.fixture(scope="module")
def scale():
    return S.scale_text()


def mask_of(contexts):
    return sum(1 << S.CONTEXTS.index(c) for c in contexts)


def insert_decided(L, r, text, mask):
    """the deferred lines through the host's parser and back into the handle"""
    ins = CX.decide(L, text, r.deferred(), mask)
    if mask == 1:
        r.insert(*ins[:8])
    else:
        r.insert(*ins[:8], context=ins[8])
    return len(ins[0])


def chunk_records(text, lines, slab_bytes):
    """the records of every chunk, from the file lines of the records"""
    cuts = S.slabs(text, slab_bytes)
    first = np.array([text.count(b"\n", 0, b) for b, _ in cuts] + [text.count(b"\n")], dtype=np.int64)
    return np.diff(np.searchsorted(lines, first))


def assert_same_arrays(got, want, keys):
    for k in keys:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), k


def check_parse(gpu_ctx, L, scale, contexts, slab_bytes):
    """Context.parse_sites and parse_sites_resident of the scale text against its truth"""
    text, truth, planted = scale
    mask = mask_of(contexts)
    decided, whole = S.truth_under(truth, mask, decided_only=True), S.truth_under(truth, mask)
    want_deferred = S.deferred_under(planted, mask)
    assert 0.99 * len(whole["line"]) <= len(decided["line"]) < len(whole["line"])
    sites, deferred = gpu_ctx.parse_sites(text, slab_bytes=slab_bytes, contexts=contexts)
    P.assert_sites_equal(sites, decided, KEYS + (["context"] if mask != 1 else []))
    assert sites["n_lines"] == planted["n_lines"]
    assert_same_arrays(deferred, want_deferred, ("line", "offset", "length"))
    r = gpu_ctx.parse_sites_resident(text, slab_bytes=slab_bytes, contexts=contexts)
    try:
        info = r.info()
        assert (info["n_sites"], info["n_deferred"], info["n_lines"]) == (len(decided["line"]), len(want_deferred["line"]),
                                                                          planted["n_lines"])
        P.assert_sites_equal(r.fetch(), decided, KEYS)
        assert r.contexts().tobytes() == decided["context"].tobytes() and r.mask() == mask
        assert_same_arrays(r.deferred(), want_deferred, ("line", "offset", "length"))
        assert insert_decided(L, r, text, mask) == len(whole["line"]) - len(decided["line"])
        P.assert_sites_equal(r.fetch(), whole, KEYS)
        assert r.contexts().tobytes() == whole["context"].tobytes()
        flagged = r.flagged()
        assert flagged.dtype == np.int64 and flagged.tolist() == planted["flagged"].tolist()
        info = r.info()
        assert (info["n_sites"], info["n_deferred"], info["n_lines"]) == (len(whole["line"]), len(want_deferred["line"]),
                                                                          planted["n_lines"])
    finally:
        r.close()
    return decided


# ---------------------------------------------------------------- 1. one slab past every parse threshold
@pytest.mark.parametrize("contexts", [("CG",), S.CONTEXTS], ids=["CG", "all"])
def test_one_slab_past_every_parse_threshold(gpu_ctx, L, scale, contexts):
    text, truth, planted = scale
    n_blocks, n_runs = S.k1_blocks(len(text)), S.ceil_div(planted["n_lines"] - 1, S.PARSE_RUN)
    assert n_blocks > S.PARSE_SCAN_THREADS and S.scan_per(n_blocks, S.PARSE_SCAN_THREADS) == 4      # K1's counts
    assert n_blocks % 4 != 0                                                                       # a ragged last slice
    assert n_runs > S.PARSE_SCAN_THREADS and S.scan_per(n_runs, S.PARSE_SCAN_THREADS) == 2          # K3's counts
    assert S.ceil_div(n_runs, 2) < S.PARSE_SCAN_THREADS                                             # lanes with empty slices
    decided = check_parse(gpu_ctx, L, scale, contexts, 0)
    assert len(decided["line"]) > S.FLAG_TRIP                                 # the flag kernel's second trip, in one chunk
    rec_flagged = np.flatnonzero(decided["status_flag"])
    assert rec_flagged[0] < S.FLAG_TRIP <= rec_flagged[-1]                    # flagged records in both trips
    if contexts == ("CG",):                                                   # the first, the last, either side of the second trip
        assert {0, S.FLAG_TRIP - 1, S.FLAG_TRIP, len(decided["line"]) - 1} <= set(rec_flagged.tolist())


# ---------------------------------------------------------------- 2. slabs
@pytest.mark.parametrize("contexts", [("CG",), S.CONTEXTS], ids=["CG", "all"])
def test_slabs_of_more_than_1024_blocks(gpu_ctx, L, scale, contexts):
    text, truth, planted = scale
    cuts = S.slabs(text, S.SLAB_BYTES)
    assert len(cuts) == 3
    assert all(S.scan_per(S.k1_blocks(e - b), S.PARSE_SCAN_THREADS) == 2 for b, e in cuts[:2])
    decided = S.truth_under(truth, mask_of(contexts), decided_only=True)
    per_chunk = chunk_records(text, decided["line"], S.SLAB_BYTES)
    assert per_chunk.sum() == len(decided["line"]) and per_chunk.min() > 0
    if contexts == ("CG",):
        assert per_chunk.max() <= S.FLAG_TRIP                                 # no chunk with a second flag trip
    check_parse(gpu_ctx, L, scale, contexts, S.SLAB_BYTES)


# ---------------------------------------------------------------- 3. split
@pytest.mark.parametrize("slab_bytes", [0, S.SLAB_BYTES], ids=["one chunk", "slabs"])
def test_split_of_more_than_1024_workgroups(gpu_ctx, L, scale, slab_bytes):
    text, truth, planted = scale
    decided = S.truth_under(truth, 7, decided_only=True)
    per_chunk = chunk_records(text, decided["line"], slab_bytes)
    groups = int(np.sum(-(-per_chunk // S.SPLIT_THREADS)))
    assert groups > S.PARSE_SCAN_THREADS and S.scan_per(groups, S.PARSE_SCAN_THREADS) == 2
    assert len(per_chunk) == (3 if slab_bytes else 1)                         # slabs: block0 != 0 in the later chunks
    parent = gpu_ctx.parse_sites_resident(text, slab_bytes=slab_bytes, contexts=S.CONTEXTS)
    children = {}
    try:
        assert insert_decided(L, parent, text, 7) > 100
        children = parent.split()
        assert list(children) == list(S.CONTEXTS)
        for c, (name, child) in enumerate(children.items()):
            want = S.truth_under(truth, 1 << c)
            assert len(want["line"]) > S.FLAG_TRIP
            P.assert_sites_equal(child.fetch(), want, KEYS)
            assert child.contexts().tobytes() == want["context"].tobytes() and child.mask() == 1 << c, name
            flagged = child.flagged()
            assert flagged.dtype == np.int64 and flagged.tolist() == want["line"][want["status_flag"] != 0].tolist(), name
            info = child.info()
            assert (info["n_sites"], info["n_deferred"], info["n_lines"]) == (len(want["line"]), 0, planted["n_lines"]), name
        assert len(children["CG"].flagged()) == len(planted["flagged"]) and len(children["CHH"].flagged()) == 0
        P.assert_sites_equal(parent.fetch(), S.truth_under(truth, 7), KEYS)   # the parent is not consumed
    finally:
        for child in children.values():
            child.close()
        parent.close()


# ---------------------------------------------------------------- 4. alignment, arrays in
@pytest.mark.parametrize("name,args,per_position,per_union", S.alignment_cases(), ids=[c[0] for c in S.alignment_cases()])
def test_alignments_past_the_common_scan(gpu_ctx, name, args, per_position, per_union):
    off, chrom, start, end, strand, _, want = S.scale_keys(**args)
    assert S.alignment_pers(off) == (per_position, per_union)                 # per = 1: the control beside its neighbour
    if "probe" in name:
        probe = int(np.argmin(np.diff(off)))
        assert probe != 0 and S.ceil_div(int(np.diff(off)[probe]), S.COMMON_THREADS) == S.COMMON_THREADS + (per_position - 1)
    if "union of" in name:
        assert S.ceil_div(int(off[-1]), S.COMMON_THREADS) == S.COMMON_THREADS + (per_union - 1)
    keep, n_common = gpu_ctx.common_sites(off, chrom, start, end, strand)
    assert n_common == want["n_common"] and keep.dtype == np.uint8 and keep.tobytes() == want["keep"].tobytes()
    dest, n_union = gpu_ctx.union_sites(off, chrom, start, end, strand)
    assert n_union == want["n_union"] and dest.dtype == np.uint32 and dest.tobytes() == want["dest"].tobytes()
    if args.get("disjoint_last_run"):
        assert not keep[chrom == S.CHROMOSOMES[-1][1]].any() and 0 < n_common


# ---------------------------------------------------------------- 5. handles at scale
@pytest.fixture(scope="module")
def samples(gpu_ctx, L):
    """the three samples of test 4 as all-CG texts, parsed resident with their deferred lines inserted; per sample the
    model's arrays: the keys, the code byte, counted and the level of every site"""
    name, args, per_position, per_union = S.alignment_cases()[0]
    off, chrom, start, end, strand, _, want = S.scale_keys(**args)
    assert S.alignment_pers(off) == (2, 4) and len(off) == 4
    made = {"off": off, "want": want, "sites": [], "model": []}
    for s in range(3):
        k = slice(off[s], off[s + 1])
        text, values = S.keys_text(chrom[k], start[k], strand[k], seed=50 + s)
        r = gpu_ctx.parse_sites_resident(text)
        made["sites"].append(r)
        assert r.info()["n_sites"] > S.FLAG_TRIP and r.info()["n_deferred"] >= 4      # records past the flag kernel's first trip
        assert insert_decided(L, r, text, 1) == r.info()["n_deferred"]
        assert r.info()["n_sites"] == off[s + 1] - off[s]
        made["model"].append({"chromosome": chrom[k], "start": start[k], "code": K.code_bytes(values["status"], values["posteriormax"]),
                              "counted": K.counted(values["posteriormax"]), "level": values["meth_lvl"]})
    yield made
    for r in made["sites"]:
        r.close()


def aligned_model(samples, align):
    """-> (columns' chromosome, start, codes (3, n), counted (3, n), level (3, n), [per sample (sum, kept) of the whole row])"""
    off, want, model = samples["off"], samples["want"], samples["model"]
    if align == "position":
        keep = [want["keep"][off[s]:off[s + 1]] != 0 for s in range(3)]
        n = want["n_common"]
        chrom, start = model[0]["chromosome"][keep[0]], model[0]["start"][keep[0]]
        rows = {k: np.stack([m[k][kp] for m, kp in zip(model, keep)]) for k in ("code", "counted", "level")}
    else:
        dest = [want["dest"][off[s]:off[s + 1]] for s in range(3)]
        n = want["n_union"]
        chrom, start = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.uint32)
        rows = {"code": np.full((3, n), 0x80, dtype=np.uint8), "counted": np.zeros((3, n), dtype=bool), "level": np.zeros((3, n))}
        for s, (m, d) in enumerate(zip(model, dest)):
            chrom[d], start[d] = m["chromosome"], m["start"]
            for k in rows:
                rows[k][s, d] = m[k]
    assert rows["code"].shape == (3, n) and n > S.COMMON_TRIP
    folds = [S.fold(c, x) for c, x in zip(rows["counted"], rows["level"])]
    return chrom, start, rows["code"], rows["counted"], rows["level"], folds


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def dvalue(diff, both):
    with np.errstate(all="ignore"):
        return diff.astype(np.float64) / (2.0 * both.astype(np.float64))


@pytest.mark.parametrize("align", ["position", "union"])
def test_codes_from_samples_of_more_than_65536_sites(abn, gpu_ctx, samples, align):
    chrom, start, code, counted, level, folds = aligned_model(samples, align)
    n = code.shape[1]
    codes = abn.Codes.from_parsed(gpu_ctx, samples["sites"], posterior_max_filter=FLT, align=align)
    try:
        assert codes.info() == {"n_samples": 3, "n_sites": n, "row_stride": max(abn.packed_row_stride(n), 64), "same_len": True}
        before, each, ms = codes.common() if align == "position" else codes.union()
        assert before.tolist() == np.diff(samples["off"]).tolist() and each == n and np.all(ms > 0)
        assert codes.packed().tobytes() == K.packed_rows(abn, list(code)).tobytes()                  # padding included
        count, lsk, kept = codes.stats()
        assert count.tolist() == [n] * 3 and kept.tolist() == [k for _, k in folds] and min(kept) > 1000
        assert bits(lsk).tolist() == bits([s for s, _ in folds]).tolist()                          # the loop's bits
        table = TR.table(code)
        assert table.sum(axis=(1, 2)).min() > 1000
        got = codes.transitions()
        assert got.dtype == table.dtype and np.array_equal(got, table)
        both, diff = TR.folds(table)
        d, b, dv = codes.pairwise()
        assert d.dtype == b.dtype == np.uint64 and np.array_equal(d, diff) and np.array_equal(b, both)
        assert both.min() > 1000 and bits(dv).tolist() == bits(dvalue(diff, both)).tolist()
    finally:
        codes.close()


@pytest.mark.parametrize("align", ["position", "union"])
def test_tiles_from_samples_of_more_than_65536_sites(abn, gpu_ctx, samples, align):
    chrom, start, code, counted, level, folds = aligned_model(samples, align)
    n = code.shape[1]
    tiles = abn.Tiles.from_parsed(gpu_ctx, samples["sites"], posterior_max_filter=FLT, align=align)
    try:
        runs = S.runs_of(chrom, start)
        assert [r[0] for r in runs] == [k for _, k in S.CHROMOSOMES]
        tiles.set_fixed(TILE)
        want_tiles = T.fixed_intervals(runs, TILE)
        n_tiles = len(want_tiles[0])
        assert n_tiles > 10
        assert tiles.info() == {"n_samples": 3, "n_columns": n, "row_stride": max(abn.packed_row_stride(n), 64), "n_runs": 5,
                                "n_tiles": n_tiles}
        assert list(zip(*(a.tolist() for a in tiles.runs()))) == runs
        assert all(g.tolist() == w.tolist() for g, w in zip(tiles.intervals(), want_tiles))
        begin, end = tiles.layout()
        want_begin, want_end = S.tile_search(chrom, start, want_tiles)
        assert begin.dtype == end.dtype == np.int64 and begin.tolist() == want_begin.tolist() and end.tolist() == want_end.tolist()
        assert (end - begin).sum() == n and (end - begin).max() > 1024
        count, lsk, kept = tiles.stats()
        want = [[S.fold(counted[s, b:e], level[s, b:e]) for b, e in zip(begin.tolist(), end.tolist())] for s in range(3)]
        assert count.tolist() == (end - begin).tolist()
        assert kept.tolist() == [[k for _, k in row] for row in want]
        assert bits(lsk).tolist() == bits([[x for x, _ in row] for row in want]).tolist()
        assert kept.sum(axis=1).tolist() == [k for _, k in folds]
        table = TR.windows_table(code, begin, end)
        got = tiles.transitions()
        assert got.dtype == table.dtype and np.array_equal(got, table)
        both, diff = TR.folds(table)
        d, b, dv = tiles.pairwise()
        assert d.dtype == b.dtype == np.uint64 and np.array_equal(d, diff) and np.array_equal(b, both) and np.median(both) > 100
        assert np.array_equal(dv, dvalue(diff, both), equal_nan=True)
    finally:
        tiles.close()
