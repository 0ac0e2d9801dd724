"""The scale tier without a GPU: the constants tests/_scale_model.py derives its sizes from are the headers', its float
tokens are all of the kind the device decides, the host parsers read its texts as exactly the arrays they were written
from, and the serial host forms of the split, the merge and the two alignments give that truth at the sizes
tests/test_scale_gpu.py runs on the device.  The vectorised models are pinned to the per-site ones at their own shapes."""
import ctypes as C
import re
import struct
from pathlib import Path

import numpy as np
import pytest

import _codes_model as K
import _common_model as X
import _contexts_model as CX
import _parse_model as P
import _scale_model as S
import _tiles_model as T
import _union_model as U
import _windows_model as M
import test_sites_merge_cpu as MERGE
from test_sites_split_cpu import split_serial

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "alphabeta_rs_amd" / "csrc"
RECORD_KEYS = [k for k, _ in P.FIELDS]


@pytest.fixture(scope="module")
def L():
    return CX.hostlib()


@pytest.fixture(scope="module")
def A():
    """the serial forms of the two alignments, arrays in"""
    L = M.hostlib()
    ll, p = C.c_longlong, C.POINTER
    L.abh_sites_common_serial.argtypes = [C.c_int, p(ll), p(C.c_int), p(C.c_uint), p(C.c_uint), p(C.c_ubyte), p(C.c_ubyte),
                                          p(ll), C.c_char_p, ll]
    L.abh_sites_common_serial.restype = ll
    L.abh_sites_union_serial.argtypes = [C.c_int, p(ll), p(C.c_int), p(C.c_uint), p(C.c_uint), p(C.c_ubyte), p(C.c_uint), p(ll),
                                         C.c_char_p, ll, ll, p(C.c_ubyte), p(C.c_double), p(C.c_int), p(C.c_uint), p(C.c_uint),
                                         p(C.c_ubyte), p(C.c_ubyte), p(C.c_double)]
    L.abh_sites_union_serial.restype = ll
    return L


# ---------------------------------------------------------------- the thresholds
def test_constants_are_the_headers():
    assert sorted(S.CONSTANTS) == ["COMMON_THREADS", "MERGE_FLAG_BLOCKS", "MERGE_THREADS", "PARSE_PIECE_BYTES", "PARSE_RUN",
                                   "PARSE_SCAN_THREADS", "PARSE_THREADS", "SPLIT_THREADS"]
    for name, (header, cxx) in S.CONSTANTS.items():
        found = re.findall(rf"constexpr\s+int\s+{cxx}\s*=\s*(\d+)\s*;", (CSRC / header).read_text())
        assert len(found) == 1 and int(found[0]) == getattr(S, name), (name, header, cxx, found)
    # the sizes of tests/test_scale_gpu.py as the issue states them
    assert S.SCALE_LINES == 262401 and S.FLAG_TRIP == S.COMMON_TRIP == 65536
    assert S.scan_per(S.ceil_div(S.SCALE_LINES, S.PARSE_RUN), S.PARSE_SCAN_THREADS) == 2
    assert S.ceil_div(1026, 2) == 513                                          # lanes 513 to 1023: empty slices


# ---------------------------------------------------------------- the float tokens
def test_every_pool_token_is_a_value_the_device_decides(L):
    tokens, values, classes = S.token_pool()
    assert 4000 <= len(tokens) <= 4200 and len(set(S.BOUNDARY_TOKENS)) == 9 and set(S.BOUNDARY_TOKENS) <= set(tokens)
    for c in range(4):
        assert np.count_nonzero(classes == c) >= 0.2 * len(tokens), S.POOL_CLASSES[c]
    for tok, want in zip(tokens, values.tolist()):
        cls, got = P.token_class(L, tok.encode())
        assert cls == P.VALUE and P.bits(got) == P.bits(want) == P.bits(float(tok)), tok
    for tok in S.DEFERRED_TOKENS:
        assert P.token_class(L, tok.encode())[0] == P.DEFER, tok
    # the classes are what they say: 16 significant digits in (c), an exponent in (d), negatives and zeros in (b)
    c_digits = [len(t.replace(".", "").lstrip("0")) for t, c in zip(tokens, classes) if c == 2]
    assert set(c_digits) == {16}
    b = [t for t, c in zip(tokens, classes) if c == 1]
    assert sum(t.startswith("-") for t in b) > 100 and sum(t.lstrip("-").startswith("0") for t in b) > 100
    assert sum(t.endswith("0") for t in b) > 100 and {len(t.lstrip("-").replace(".", "")) for t in b} >= set(range(1, 16))
    d = [t.lower().split("e") for t, c in zip(tokens, classes) if c == 3]
    assert {int(x) for _, x in d} == set(range(-22, 23)) and max(int(w) for w, _ in d) <= 1 << 53


# ---------------------------------------------------------------- the text of GPU tests 1 to 3
@pytest.fixture(scope="module")
def scale():
    return S.scale_text()


def test_scale_text_has_the_planted_shape(scale):
    text, truth, planted = scale
    n = S.SCALE_LINES
    assert text.count(b"\n") == n + 1 == planted["n_lines"]
    n_blocks = S.k1_blocks(len(text))
    assert n_blocks > 3 * S.PARSE_SCAN_THREADS and S.scan_per(n_blocks, S.PARSE_SCAN_THREADS) == 4      # ragged last slice
    assert n_blocks % 4 != 0
    cuts = S.slabs(text, S.SLAB_BYTES)
    assert len(cuts) == 3 and all(S.scan_per(S.k1_blocks(e - b), S.PARSE_SCAN_THREADS) == 2 for b, e in cuts[:2])
    d = set((planted["deferred"] - 1).tolist())                               # data lines
    last_run = 1024
    assert {0, n - 1, 255, 256, 257, last_run * 256 + 255, last_run * 256 + 256} <= d
    assert len(d) >= n // 2000 and len(planted["rejected"]) >= 36 and len(planted["flagged"]) >= 50
    assert {511, 512, 513, last_run * 256 - 1, last_run * 256, last_run * 256 + 1} <= set((planted["rejected"] - 1).tolist())
    cg = S.truth_under(truth, 1)
    at = np.flatnonzero(~cg["decided"])
    assert {S.FLAG_TRIP - 1, S.FLAG_TRIP, S.FLAG_TRIP + 1} <= set(at.tolist())                           # CG sites, deferred
    rec = S.truth_under(truth, 1, decided_only=True)
    assert len(rec["line"]) > S.FLAG_TRIP + 1
    f = np.flatnonzero(rec["status_flag"])
    assert {0, S.FLAG_TRIP - 1, S.FLAG_TRIP, len(rec["line"]) - 1} <= set(f.tolist())
    assert rec["line"][f].tolist() == planted["flagged"].tolist()              # no flagged line is deferred or of another context
    # contexts about equal, both strands, both formats, five runs in file order
    share = np.bincount(truth["context"], minlength=3) / len(truth["context"])
    assert np.all(np.abs(share - 1 / 3) < 0.01) and set(truth["strand"].tolist()) == {0, 1}
    c = truth["chromosome"]
    assert c[np.flatnonzero(np.r_[True, c[1:] != c[:-1]])].tolist() == [1, 10, 2, 256, 257]
    lengths = {line.count(b"\t") for line in text.split(b"\n")[1:2000]}
    assert lengths == {8, 9}
    for b, e in cuts:                                                          # no chunk with a second flag trip under CG alone
        lines = (text.count(b"\n", 0, b), text.count(b"\n", 0, e))
        assert np.count_nonzero((rec["line"] >= lines[0]) & (rec["line"] < lines[1])) <= S.FLAG_TRIP or len(cuts) == 1


@pytest.mark.parametrize("mask", [1, 2, 4, 7])
def test_host_parser_reads_the_truth(L, scale, mask):
    text, truth, planted = scale
    want = S.truth_under(truth, mask)
    got = CX.host_sites(L, text, mask)
    P.assert_sites_equal(got, want, RECORD_KEYS + ["context"])
    if mask == 1:                                                              # the parser without a mask argument
        plain, warnings = P.host_sites(L, text)
        P.assert_sites_equal(plain, want)
        assert warnings == len(planted["flagged"])


@pytest.mark.parametrize("mask", [1, 7])
def test_classifier_defers_the_planted_lines_and_decides_the_rest(L, scale, mask):
    text, truth, planted = scale
    cls, dev = CX.classify(L, text, mask)
    assert len(cls) == S.SCALE_LINES
    assert (np.flatnonzero(cls == 2) + 1).tolist() == S.deferred_under(planted, mask)["line"].tolist()
    assert not np.isin(planted["rejected"] - 1, np.flatnonzero(cls)).any()
    want = S.truth_under(truth, mask, decided_only=True)
    P.assert_sites_equal(dev, want, RECORD_KEYS + ["status_flag", "context"])
    sites = len(S.truth_under(truth, mask)["line"])
    assert len(dev["line"]) >= 0.99 * sites and len(dev["line"]) < sites
    uses = np.bincount(np.concatenate([want["pm_class"], want["ml_class"]]), minlength=5)
    assert np.all(uses[:4] >= 10000), uses
    spans = P.line_spans(text)                                                 # the planted offsets are the text's
    d = S.deferred_under(planted, mask)
    assert [spans[l] for l in d["line"].tolist()] == list(zip(d["offset"].tolist(), d["length"].tolist()))


# ---------------------------------------------------------------- the serial forms at scale
@pytest.mark.parametrize("slab_bytes", [0, S.SLAB_BYTES])
def test_serial_split_gives_the_truth_by_context(L, scale, slab_bytes):
    text, truth, planted = scale
    records = len(S.truth_under(truth, 7, decided_only=True)["line"])
    assert S.ceil_div(records, S.SPLIT_THREADS) > S.PARSE_SCAN_THREADS       # the split's scan: per = 2
    children, size, inserted = split_serial(L, text, 7, slab_bytes)
    assert sorted(children) == [0, 1, 2] and size.shape[0] == (3 if slab_bytes else 1) and set(inserted.tolist()) == {0, 1, 2}
    for c, got in children.items():
        P.assert_sites_equal(got, S.truth_under(truth, 1 << c), RECORD_KEYS + ["context"])


@pytest.mark.parametrize("chunk_lines", [0, 100000])
def test_serial_merge_gives_the_truth(scale, chunk_lines):
    text, truth, planted = scale
    cg = S.truth_under(truth, 1)
    n = planted["n_lines"]
    kind = np.full(n, MERGE.NOTHING)
    kind[cg["line"]] = np.where(cg["decided"], MERGE.RECORD, MERGE.ACCEPTED)
    f = {"chromosome": np.zeros(n, dtype=np.int32), "start": np.zeros(n, dtype=np.uint32), "end": np.zeros(n, dtype=np.uint32),
         "strand": np.zeros(n, dtype=np.uint8), "status": np.zeros(n, dtype=np.uint8), "flag": np.zeros(n, dtype=np.uint32),
         "pm": np.zeros(n), "ml": np.zeros(n)}
    for k, t in (("chromosome", "chromosome"), ("start", "start"), ("end", "end"), ("strand", "strand"), ("status", "status"),
                 ("flag", "status_flag"), ("pm", "posteriormax"), ("ml", "meth_lvl")):
        f[k][cg["line"]] = cg[t]
    n_rec, n_ins, _ = MERGE.check(MERGE.hostlib(), kind, f, chunk_lines, chunk_lines)
    assert n_rec > S.FLAG_TRIP and n_ins >= 10


def common_serial(A, off, chrom, start, end, strand):
    t = A.abh_sites_common_serial.argtypes
    keep = np.full(max(int(off[-1]), 1), 7, dtype=np.uint8)
    refusal, text = np.zeros(3, dtype=np.int64), C.create_string_buffer(256)
    n = A.abh_sites_common_serial(len(off) - 1, *(np.ascontiguousarray(a).ctypes.data_as(ty) for a, ty in
                                                  zip((off, chrom, start, end, strand), t[1:6])),
                                  keep.ctypes.data_as(t[6]), refusal.ctypes.data_as(t[7]), text, len(text))
    assert n >= 0, text.value
    return keep[:int(off[-1])], n


def union_serial(A, off, chrom, start, end, strand):
    t = A.abh_sites_union_serial.argtypes
    dest = np.full(max(int(off[-1]), 1), 0xdeadbeef, dtype=np.uint32)
    refusal, text = np.zeros(3, dtype=np.int64), C.create_string_buffer(256)
    n = A.abh_sites_union_serial(len(off) - 1, *(np.ascontiguousarray(a).ctypes.data_as(ty) for a, ty in
                                                 zip((off, chrom, start, end, strand), t[1:6])),
                                 dest.ctypes.data_as(t[6]), refusal.ctypes.data_as(t[7]), text, len(text), 0, *[None] * 8)
    assert n >= 0, text.value
    return dest[:int(off[-1])], n


@pytest.mark.parametrize("name,args,per_position,per_union", S.alignment_cases(), ids=[c[0] for c in S.alignment_cases()])
def test_serial_alignments_give_the_set_operations(A, name, args, per_position, per_union):
    off, chrom, start, end, strand, index, want = S.scale_keys(**args)
    assert np.diff(off).tolist() == list(args["kept"]) and S.alignment_pers(off) == (per_position, per_union)
    keep, n_common = common_serial(A, off, chrom, start, end, strand)
    assert n_common == want["n_common"] and keep.tobytes() == want["keep"].tobytes()
    dest, n_union = union_serial(A, off, chrom, start, end, strand)
    assert n_union == want["n_union"] and dest.tobytes() == want["dest"].tobytes()
    assert 0 < n_common < np.diff(off).min() and n_union > np.diff(off).max()
    same_start = np.flatnonzero((start[1:] == start[:-1]) & (chrom[1:] == chrom[:-1]))
    assert len(same_start) > 100 and np.all(strand[same_start] < strand[same_start + 1])      # both strands at one start
    if args.get("disjoint_last_run"):
        assert not keep[chrom == S.CHROMOSOMES[-1][1]].any() and (chrom == S.CHROMOSOMES[-1][1]).sum() > 300
        assert np.argmin(np.diff(off)) == 1                                    # not sample 0 is the shortest


# ---------------------------------------------------------------- the vectorised models against the per-site ones
def test_expected_alignment_equals_the_set_models_at_their_shapes():
    rng = np.random.default_rng(20261019)
    cases = []
    for n_common in (0, 1, 63, 64, 65, 255, 256, 257, 1025):
        for n_samples in (1, 2, 3, 5):
            cases.append(X.make_case(rng, n_samples, n_common, (0, 7, 40)[(n_common + n_samples) % 3],
                                     chrom_order=((1, 10, 2), (2, 1, 257, 256))[n_samples % 2], lonely=(None, 30)[n_common % 2],
                                     drop_first=n_common % 3 == 0, drop_last=n_common % 3 == 1))
    cases += [samples for _, samples, _ in U.generated_cases()]
    assert len(cases) == 36 + 108
    for samples in cases:
        keep, n_common, dest, n_union = S.expected_alignment(*X.concat(samples))
        common, union = X.model(samples), U.model(samples)
        assert common[0] == union[0] == "ok"
        assert n_common == common[2] and keep.tobytes() == np.concatenate(common[1] + [np.zeros(0, dtype=np.uint8)]).tobytes()
        assert n_union == union[2] and dest.tobytes() == np.concatenate(union[1] + [np.zeros(0, dtype=np.uint32)]).tobytes()


def test_vectorised_fold_and_tile_search_equal_the_loops():
    rng = np.random.default_rng(3)
    for n in (0, 1, 2, 17, 256, 3000):
        pm = np.where(rng.random(n) < 0.5, 0.99, rng.random(n))
        ml = np.where(rng.random(n) < 0.2, -0.0, rng.random(n) * 10.0 ** rng.integers(-5, 6, size=n))
        for level in (ml, np.full(n, -0.0)):
            s, k = S.fold(K.counted(pm), level)
            assert (struct.pack("<d", s), k) == K.fold(pm, level) == T.fold(K.counted(pm), level, 0, n)
    assert S.fold(np.zeros(5, dtype=bool), np.ones(5)) == (0.0, 0) and struct.pack("<d", S.fold([True], [-0.0])[0]) == struct.pack("<d", 0.0)
    rows = T.master_sites()
    chrom = np.array([T.chromosome_key(r[0]) for r in rows], dtype=np.int32)
    start = np.array([r[1] for r in rows], dtype=np.int64)
    explicit, _ = T.tile_list(rows)
    assert S.runs_of(chrom, start) == T.runs_of(chrom, start) and S.runs_of([], []) == T.runs_of([], []) == []
    fixed = T.fixed_intervals(T.runs_of(chrom, start), 1 << 28)
    for tiles in (explicit, fixed):
        for got, want in zip(S.tile_search(chrom, start, tiles), T.search(chrom, start, tiles)):
            assert got.dtype == want.dtype and got.tolist() == want.tolist()


def test_keys_text_is_read_as_its_arrays(L):
    off, chrom, start, end, strand, index, _ = S.scale_keys(seed=9, universe=3000, kept=(2900,))
    text, values = S.keys_text(chrom, start, strand, seed=9)
    got, _ = P.host_sites(L, text)
    want = {"line": np.arange(1, 2901, dtype=np.int64), "chromosome": chrom, "start": start, "end": end, "strand": strand, **values}
    P.assert_sites_equal(got, want)
    cls, _ = P.classify(L, text)
    assert 2 <= np.count_nonzero(cls == 2) <= 42 and np.count_nonzero(cls == 1) + np.count_nonzero(cls == 2) == 2900
    assert 0.5 < K.counted(values["posteriormax"]).mean() < 0.9
