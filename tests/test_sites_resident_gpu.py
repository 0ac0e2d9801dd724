"""Parse results resident on the device (abn_sites_parse_dev, abn_sites_insert, abn_windows_create_parsed;
alphabeta_rs_amd/csrc/abn_sites_merge.hpp) against the host-resident forms: the fetched records bit for bit, the window
handle in everything it reports, and `metaprofile_alphabeta --sites device` file for file."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import _contexts_model as X
import _genes_model as G
import _parse_model as P
import _windows_model as M

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden"
FLT = 0.99
KEYS = [k for k, _ in P.FIELDS] + ["status_flag"]
LONG = "0.999900000000000000000"      # 21 digits: the device defers the line, the host reads 0.9999


@pytest.fixture(scope="module")
def L():
    L = P.hostlib()
    L.abh_parse_sites_resident.argtypes = L.abh_parse_sites_device.argtypes
    L.abh_parse_sites_resident.restype = C.c_longlong
    return L


def decide(L, text, deferred):
    """parse_site_full on every deferred line -> the arrays Sites.insert takes"""
    rows = []
    for line, off, n in zip(*(deferred[k].tolist() for k in ("line", "offset", "length"))):
        s, _ = P.host_sites(L, text[off:off + n], skip_lines=0)
        assert len(s["line"]) <= 1
        if len(s["line"]):
            rows.append((line, *(s[k][0] for k in ("chromosome", "start", "end", "strand", "posteriormax", "status", "meth_lvl"))))
    cols = list(zip(*rows)) if rows else [[]] * 8
    return [np.array(c, dtype=t) for c, t in zip(cols, (np.int64, np.int32, np.uint32, np.uint32, np.uint8, np.float64,
                                                        np.uint8, np.float64))]


def resident(ctx, L, text, slab_bytes=0):
    """parse_sites_resident with the host-decided lines inserted"""
    r = ctx.parse_sites_resident(text, slab_bytes=slab_bytes)
    r.insert(*decide(L, text, r.deferred()))
    return r


def host_layer_resident(L, text, slab_bytes):
    """windows::parse_sites_resident of the host layer -> (what its handle fetches, the warnings it printed)"""
    cap = text.count(b"\n") + 2
    arrays, ptrs = P._site_arrays(L, cap)
    warn = C.create_string_buffer(1 << 16)
    n = L.abh_parse_sites_resident(text, len(text), 1, slab_bytes, cap, *ptrs, warn, len(warn))
    assert n >= 0, n
    return {k: a[:n] for k, a in arrays.items()}, warn.value.decode(errors="replace")


FETCH_TEXTS = ([("methylome " + p.name, p.read_bytes()) for p in P.GOLDEN_METHYLOMES] + [("torture", P.torture_text())] +
               [(f"plain {n}", P.plain_text(n, seed=n, cg_every=2)) for n in (255, 256, 257, 1025)])


@pytest.mark.parametrize("slab_bytes", [0, 4096, 300])
def test_resident_fetch_equals_host_form(gpu_ctx, L, slab_bytes):
    assert len(FETCH_TEXTS) >= 6
    n_deferred = n_inserted = 0
    for name, text in FETCH_TEXTS:
        sites, deferred = gpu_ctx.parse_sites(text, slab_bytes=slab_bytes)
        r = gpu_ctx.parse_sites_resident(text, slab_bytes=slab_bytes)
        try:
            info = r.info()
            assert (info["n_sites"], info["n_deferred"], info["n_lines"]) == (len(sites["line"]), len(deferred["line"]), sites["n_lines"]), name
            assert info["kernel_ms"] > 0.0 or len(text) == 0
            P.assert_sites_equal(r.fetch(), sites, KEYS)
            got = r.deferred()
            assert all(got[k].dtype == deferred[k].dtype and np.array_equal(got[k], deferred[k]) for k in deferred), name
            ins = decide(L, text, got)
            r.insert(*ins)
            merged, warnings = P.device_sites_merged(L, text, 1, slab_bytes)
            assert r.info()["n_sites"] == len(merged["line"]) == len(sites["line"]) + len(ins[0]), name
            P.assert_sites_equal(r.fetch(), merged)
            assert np.array_equal(r.fetch()["status_flag"] != 0, np.isin(merged["line"], r.flagged())), name
            layer, layer_warnings = host_layer_resident(L, text, slab_bytes)      # the host layer's own walk
            P.assert_sites_equal(layer, merged)
            assert layer_warnings == warnings, name
            n_deferred += len(got["line"])
            n_inserted += len(ins[0])
        finally:
            r.close()
    assert 0 < n_inserted < n_deferred          # the torture text: deferred lines of both outcomes


# ---------------------------------------------------------------- abn_sites_fetch with some outputs null
def partial_fetch_texts():
    """the torture text (deferred lines of both outcomes) and 257 plain lines with the first and last line of two of the
    300-byte slabs deferred"""
    d = Deferring(P.plain_text(257, seed=257, cg_every=2).decode())
    d.slab = 300
    for chunk in (1, 3):
        d.mark_chunk_edges(chunk)
    assert min(d.at_edges()) >= 2
    return (("torture", P.torture_text()), ("plain 257", d.text()))


def check_partial_fetches(lib, r, name):
    """abn_sites_fetch with one output non-null at a time, and with the three the host layer reads (host/resident.hpp):
    each column is the full fetch()'s, and no other array is written"""
    want = r.fetch()
    n = len(want["line"])
    assert r.contexts().shape == (n,)
    kinds = list(r.KINDS.items())
    types = lib.abn_sites_fetch.argtypes[1:]
    for asked in [(k,) for k, _ in kinds] + [("posteriormax", "status", "meth_lvl")]:
        got = {k: np.full(n + 1, 0x5a, dtype=t) for k, t in kinds}      # one element more: nothing is written behind the end
        rc = lib.abn_sites_fetch(r._h, *(got[k].ctypes.data_as(t) if k in asked else None for (k, _), t in zip(kinds, types)))
        assert rc == 0, (name, asked)
        for k, t in kinds:
            if k in asked:
                assert got[k].dtype == want[k].dtype and got[k][:n].tobytes() == want[k].tobytes(), (name, asked, k)
                assert got[k][n] == t(0x5a), (name, asked, k)
            else:
                assert np.all(got[k] == t(0x5a)), (name, asked, k)
    codes = np.full(n + 1, 0x5a, dtype=np.uint8)                         # the tenth column: abn_sites_context
    assert lib.abn_sites_context(r._h, None, codes.ctypes.data_as(C.POINTER(C.c_uint8))) == 0
    assert codes[:n].tobytes() == r.contexts().tobytes() and codes[n] == 0x5a, name
    return n


@pytest.mark.parametrize("contexts", [("CG",), X.CONTEXTS])
def test_fetch_with_some_outputs_null(gpu_ctx, L, contexts):
    lib = gpu_ctx._L
    XL = X.hostlib()
    n_inserted = n_child_inserted = 0
    for name, text in partial_fetch_texts():
        r = gpu_ctx.parse_sites_resident(text, slab_bytes=300, contexts=contexts)
        children = {}
        try:
            if len(contexts) == 1:
                ins = decide(L, text, r.deferred())
                r.insert(*ins)
                P.assert_sites_equal(r.fetch(), P.device_sites_merged(L, text, 1, 300)[0])
            else:
                ins = X.decide(XL, text, r.deferred(), 7)
                r.insert(*ins[:8], context=ins[8])
                host = X.host_sites(XL, text, 7)
                P.assert_sites_equal(r.fetch(), host)
                assert r.contexts().tobytes() == host["context"].tobytes(), name
            assert len(ins[0]) > 0 and len(slabs(text, 300)) > 3, name
            n_inserted += len(ins[0])
            assert check_partial_fetches(lib, r, name) == r.info()["n_sites"]
            if len(contexts) > 1:
                children = r.split()
                assert list(children) == list(X.CONTEXTS)
                codes = r.contexts()
                for c, child in enumerate(children.values()):
                    n = check_partial_fetches(lib, child, (name, c))
                    assert n == np.count_nonzero((codes == c) | (codes == 3)), (name, c)
                    assert np.all(np.isin(child.contexts(), (c, 3)))
                    n_child_inserted += int(np.count_nonzero((ins[8] == c) | (ins[8] == 3)))
        finally:
            for s in children.values():
                s.close()
            r.close()
    assert n_inserted >= 8 and (len(contexts) == 1 or n_child_inserted >= 8)


# ---------------------------------------------------------------- the window handle
def slabs(text, slab_bytes):
    """[(first line, last line)] of the slabs abn_sites_parse cuts: behind the last line end of every slab_bytes bytes, or —
    a line longer than that — behind that line"""
    out, at, line = [], 0, 0
    while at < len(text):
        if len(text) - at <= slab_bytes:
            end = len(text)
        else:
            cut = text.rfind(b"\n", at, at + slab_bytes)
            if cut < 0:
                cut = text.find(b"\n", at + slab_bytes)
            end = len(text) if cut < 0 else cut + 1
        n = text.count(b"\n", at, end) + (0 if text[end - 1:end] == b"\n" else 1)
        out.append((line, line + n - 1))
        line += n
        at = end
    return out


class Deferring:
    """a methylome text whose marked lines carry a posterior token the device defers: the 21-digit spelling and `nan` in
    turn (a line without that column, a 4-field row, cannot be marked)"""

    def __init__(self, text):
        self.lines = text.split("\n")[:-1]
        self.marked = set()
        self.slab = max(64, len(text) // 4)      # at least three slabs wherever the text has a few lines

    def mark(self, i):
        if i == 0 or i >= len(self.lines) or i in self.marked:
            return i in self.marked
        f = self.lines[i].split("\t")
        if len(f) < 9:
            return False
        f[6] = (LONG, "nan")[len(self.marked) % 2]
        self.lines[i] = "\t".join(f)
        self.marked.add(i)
        return True

    def text(self):
        return ("\n".join(self.lines) + "\n").encode()

    def mark_chunk_edges(self, chunk):
        """the first and the last line of slab `chunk`, re-cut after every mark (a longer line moves the cut); a last line
        pushed over the cut is the next slab's first: marked all the same"""
        cut = slabs(self.text(), self.slab)
        if chunk >= len(cut):
            return
        self.mark(cut[chunk][0])
        for _ in range(8):
            last = slabs(self.text(), self.slab)[chunk][1]
            if last in self.marked or not self.mark(last):
                break

    def at_edges(self):
        cut = slabs(self.text(), self.slab)
        return (sum(a in self.marked for a, _ in cut), sum(b in self.marked for _, b in cut))


def window_samples():
    """[(name, annotation, args, [Deferring text per sample])]: the hand cases of the gene choice on 1 to 4 samples and one
    seeded case with a sample of 2755 sites"""
    hand = G.hand_cases()
    cases = [(name, c.annotation, c.args, c.texts[-4:]) for name, c in hand.items()]
    seeded = G.random_case(2028, 3000, 80)
    assert [t.count("\n") - 1 for t in seeded.texts] == [1333, 2755]
    cases.append(("seeded", seeded.annotation, seeded.args, seeded.texts))
    return [(name, ann, args, [Deferring(t) for t in texts]) for name, ann, args, texts in cases]


def test_windows_from_parsed_equals_from_sites(abn, gpu_ctx, L):
    first = last = adjacent = whole = 0
    for name, ann, case_args, samples in window_samples():
        assert 1 <= len(samples) <= 4
        smallest = min((d for d in samples if len(d.lines) > 1), key=lambda d: len(d.lines))
        for d in samples:
            n = len(d.lines)
            if d is smallest and len(samples) > 1:
                whole += all([d.mark(i) for i in range(1, n)])                  # all lines of one sample
                continue
            for chunk in (0, 1, 2):
                d.mark_chunk_edges(chunk)
            if n > 40:
                adjacent += d.mark(n // 2) and d.mark(n // 2 + 1)
            a, b = d.at_edges()
            first, last = first + a, last + b
        args = M.Args(cutoff=case_args.cutoff, step=5, size=5, absolute=False, cutoff_gene_length=case_args.cutoff_gene_length, flt=FLT)
        kw = dict(cutoff=args.cutoff, cutoff_gene_length=args.cutoff_gene_length, step=args.step, size=args.size,
                  absolute=args.absolute, counts=M.windows_new(args, 100))
        genome, _ = M.genome_of(ann)
        texts = [d.text() for d in samples]
        merged = [P.device_sites_merged(L, t)[0] for t in texts]                # the merged host sequence
        for d, m in zip(samples, merged):
            assert set(d.marked) <= set(m["line"].tolist())                    # every marked line is a site the host accepts
        off = np.zeros(len(texts) + 1, dtype=np.int64)
        off[1:] = np.cumsum([len(m["line"]) for m in merged])
        cat = lambda k: np.concatenate([m[k] for m in merged])
        with np.errstate(invalid="ignore"):
            code = (cat("status") | np.where(cat("posteriormax") < FLT, 0x80, 0)).astype(np.uint8)
        genes = abn.Genes(gpu_ctx, G.gene_lists(genome))
        sites = [resident(gpu_ctx, L, t, d.slab) for t, d in zip(texts, samples)]
        a = abn.Windows.from_sites(gpu_ctx, genes, off, cat("chromosome"), cat("start"), cat("end"), cat("strand"), code,
                                   cat("meth_lvl"), **kw)
        b = abn.Windows.from_parsed(gpu_ctx, genes, sites, posterior_max_filter=FLT, **kw)
        try:
            for d, s in zip(samples, sites):
                assert s.info()["n_deferred"] >= len(d.marked)
                assert len(d.lines) < 8 or len(slabs(d.text(), d.slab)) >= 3, name
            assert (b.W, b.row_stride, b.n_sites, b.n_samples) == (a.W, a.row_stride, a.n_sites, a.n_samples), name
            for x, y in zip(a.stats() + a.layout(), b.stats() + b.layout()):     # counts, sums bit for bit, kept; layout, ragged
                assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), name
            assert np.array_equal(a.packed(), b.packed()), name
            for x, y in zip(a.pairwise(), b.pairwise()):
                assert x.tobytes() == y.tobytes(), name
            assert np.all(b.merge_ms() > 0) and not a.merge_ms().any()
            b2 = abn.Windows.from_parsed(gpu_ctx, genes, sites, posterior_max_filter=FLT, **kw)   # the handles are not consumed
            assert np.array_equal(b2.packed(), b.packed())
            b2.close()
            if name == "seeded":
                assert a.stats()[0].sum() > 1000 and np.diff(off).max() > 2 * 1024
        finally:
            a.close()
            b.close()
            genes.close()
            for s in sites:
                s.close()
    assert first >= 3 and last >= 3 and adjacent >= 3 and whole >= 2, (first, last, adjacent, whole)


def test_zero_sites_and_zero_samples_of_sites(abn, gpu_ctx, L):
    """a sample of zero sites beside one with sites, and zero sites in all: as Windows.from_sites"""
    ann = G.gene_line(1, 1000, 3000, "+")
    args = M.Args(cutoff=100, step=5, size=5)
    kw = dict(cutoff=100, step=5, size=5, absolute=False, counts=M.windows_new(args, 100))
    genes = abn.Genes(gpu_ctx, G.gene_lists(M.genome_of(ann)[0]))
    empty, some = G.text([]).encode(), G.text([G.cg(1, 1000 + 7 * i, "+") for i in range(300)]).encode()
    for texts in ([empty, some, empty], [empty], [empty, empty]):
        sites = [resident(gpu_ctx, L, t, 300) for t in texts]
        merged = [P.device_sites_merged(L, t)[0] for t in texts]
        off = np.zeros(len(texts) + 1, dtype=np.int64)
        off[1:] = np.cumsum([len(m["line"]) for m in merged])
        cat = lambda k: np.concatenate([m[k] for m in merged])
        a = abn.Windows.from_sites(gpu_ctx, genes, off, cat("chromosome"), cat("start"), cat("end"), cat("strand"),
                                   (cat("status") | np.where(cat("posteriormax") < FLT, 0x80, 0)).astype(np.uint8), cat("meth_lvl"), **kw)
        b = abn.Windows.from_parsed(gpu_ctx, genes, sites, posterior_max_filter=FLT, **kw)
        for x, y in zip(a.stats() + a.layout() + (a.packed(),), b.stats() + b.layout() + (b.packed(),)):
            assert x.dtype == y.dtype and x.tobytes() == y.tobytes()
        for h in [a, b] + sites:
            h.close()
    genes.close()


def test_flagged_lines_and_warnings(gpu_ctx, L):
    torture = P.torture_text()
    rows = [P.cg_line(pos=str(10 + i), st="UIMX?"[i % 5], tri="CGA") for i in range(700)]
    odd = (P.HEADER + "\n".join(rows) + "\n").encode()
    for text, slab_bytes in ((torture, 0), (torture, 300), (odd, 0), (odd, 4096), (odd, 300)):
        sites, _ = gpu_ctx.parse_sites(text, slab_bytes=slab_bytes)
        r = gpu_ctx.parse_sites_resident(text, slab_bytes=slab_bytes)
        flagged = r.flagged()
        r.close()
        assert flagged.dtype == np.int64 and flagged.tolist() == sites["line"][sites["status_flag"] != 0].tolist()
        assert len(flagged) >= 6
    assert len(flagged) == 2 * 700 // 5
    _, warnings = host_layer_resident(L, odd, 300)
    assert warnings.count("\n") == 280 and warnings.index("status: X") < warnings.index("status: ?")
    assert warnings == P.device_sites_merged(L, odd, 1, 300)[1]
    for n in (256, 3000):
        r = gpu_ctx.parse_sites_resident(P.plain_text(n, seed=5))
        assert len(r.flagged()) == 0 and r.info()["n_deferred"] == 0
        r.close()


def test_bad_arguments(abn, gpu_ctx, L):
    """every ABN_ERR_INVALID_ARG case of abn_sites_parse_dev, abn_sites_insert and abn_windows_create_parsed is a status
    code, and no handle comes back"""
    lib = gpu_ctx._L
    text = (P.HEADER + "\n".join([P.cg_line(pos="5"), P.cg_line(pos="6", pm=LONG), P.cg_line(pos="7"), P.cg_line(pos="8", pm="nan"),
                                  P.cg_line(pos="9", pm="abc")]) + "\n").encode()

    def parse(entry, ctx=gpu_ctx, text=text, n=None, params=None, out=True):
        h = C.c_void_p()
        rc = entry(ctx._h, text, len(text) if n is None else n, C.byref(params) if params else None, C.byref(h) if out else None)
        return rc, h

    assert parse(lib.abn_sites_parse_dev, out=False)[0] == 1
    assert parse(lib.abn_sites_parse_dev, n=-1)[0] == 1
    assert parse(lib.abn_sites_parse_dev, text=None, n=5)[0] == 1
    for bad in (abn.SitesParams(-1, 1, 0), abn.SitesParams((1 << 30) + 1, 1, 0), abn.SitesParams(0, -1, 0)):
        rc, h = parse(lib.abn_sites_parse_dev, params=bad)
        assert rc == 1 and not h.value
    assert lib.abn_sites_parse_dev(None, text, len(text), None, C.byref(C.c_void_p())) == 1

    ok = dict(line=[2, 4], chromosome=[1, 1], start=[6, 8], end=[7, 9], strand=[0, 0], posteriormax=[0.9999, np.nan],
              status=[2, 2], meth_lvl=[0.5, 0.5])

    def insert(h, **change):
        v = dict(ok, **change)
        arrays = [np.array(v[k], dtype=t) for k, t in zip(ok, (np.int64, np.int32, np.uint32, np.uint32, np.uint8, np.float64,
                                                               np.uint8, np.float64))]
        return lib.abn_sites_insert(h, len(arrays[0]), *(a.ctypes.data_as(t) for a, t in zip(arrays, lib.abn_sites_insert.argtypes[2:])))

    rc, host_form = parse(lib.abn_sites_parse)
    assert rc == 0 and insert(host_form) == 1                                      # a host-form handle
    rc, r = parse(lib.abn_sites_parse_dev)
    assert rc == 0
    nd = C.c_int64()
    assert lib.abn_sites_info(r, None, C.byref(nd), None, None) == 0 and nd.value == 3     # lines 2, 4, 5
    assert lib.abn_sites_insert(None, 0, *[None] * 8) == 1
    assert insert(r, line=[2, 3]) == 1                                              # a line that was not deferred
    assert insert(r, line=[4, 2]) == 1 and insert(r, line=[2, 2]) == 1              # unordered
    assert insert(r, chromosome=[1, 258]) == 1 and insert(r, chromosome=[-1, 1]) == 1
    assert insert(r, strand=[3, 0]) == 1 and insert(r, status=[0, 3]) == 1
    assert lib.abn_sites_insert(r, 2, *[None] * 8) == 1 and lib.abn_sites_insert(r, -1, *[None] * 8) == 1

    genes = abn.Genes(gpu_ctx, [(1, 0, [1], [100], [0])])
    p = abn.WindowsParams(100, 5, 5, 0, 20, 20, 20)
    rule = abn.GeneRule(100, 0)

    def create(handles, ctx=gpu_ctx, p=p, genes=genes._h, rule=rule, n=None, out=True):
        arr = (C.c_void_p * max(len(handles), 1))(*(h.value if isinstance(h, C.c_void_p) else h for h in handles))
        w = C.c_void_p(0xdead)
        rc = lib.abn_windows_create_parsed(ctx._h if ctx else None, C.byref(p) if p else None, genes, C.byref(rule) if rule else None,
                                           FLT, len(handles) if n is None else n, arr, C.byref(w) if out else None)
        if rc and ctx and out:
            assert not w.value
        return rc, w

    assert create([r])[0] == 1                                                      # the forgotten insert
    assert insert(r) == 0
    assert insert(r) == 1 and lib.abn_sites_insert(r, 0, *[None] * 8) == 1          # a second insert
    rc, w = create([r])
    assert rc == 0 and w.value
    lib.abn_windows_destroy(w)
    assert create([r, None])[0] == 1 and create([host_form])[0] == 1 and create([r, host_form])[0] == 1
    assert create([], n=0)[0] == 1 and create([r], n=-1)[0] == 1 and create([r], n=65536)[0] == 1
    assert create([r], ctx=None)[0] == 1 and create([r], p=None)[0] == 1 and create([r], out=False)[0] == 1
    assert create([r], genes=None)[0] == 1 and create([r], rule=None)[0] == 1
    assert create([r], p=abn.WindowsParams(100, 0, 5, 0, 20, 20, 20))[0] == 1      # what abn_windows_create_sites refuses
    assert create([r], p=abn.WindowsParams(100, 5, 5, 0, -1, 20, 20))[0] == 1
    other = abn.Context(0)
    try:
        rc, foreign = parse(lib.abn_sites_parse_dev, ctx=other, text=P.plain_text(20, seed=1))
        assert rc == 0
        assert create([foreign])[0] == 1 and create([r, foreign])[0] == 1           # a sites handle of another context
        assert create([r], ctx=other)[0] == 1                                       # (and so is r for the other one)
        lib.abn_sites_destroy(foreign)
    finally:
        other.close()
    rc, none_deferred = parse(lib.abn_sites_parse_dev, text=P.plain_text(300, seed=2))
    rc2, w = create([none_deferred, r])                                             # nothing deferred: no insert is needed
    assert (rc, rc2) == (0, 0)
    lib.abn_windows_destroy(w)
    for h in (r, host_form, none_deferred):
        assert lib.abn_sites_destroy(h) == 0
    assert lib.abn_sites_flagged(None, None, None) == 1
    genes.close()


# ---------------------------------------------------------------- the tool
def test_metaprofile_sites_device_equals_sites_host(tmp_path):
    """the fixture of tests/test_genes_gpu.py::test_metaprofile_genes_device_equals_genes_host with rows the device defers
    (both outcomes) and rows with an invalid status: every output file of --sites device is the file of --sites host, the
    warnings come in the same order; --sites device needs --parse device"""
    from alphabeta_rs_amd import build as B

    B.build_host()
    genome, genes = M.genome_of((GOLDEN / "annotation.txt").read_text())
    rng = np.random.default_rng(8)
    where = []
    for g in sorted(genes, key=lambda g: (g["chromosome"], g["start"]))[:3]:
        where += [(g, int(p)) for p in sorted(rng.integers(g["start"] - 2100, g["end"] + 2100, size=1000))]
    names = ["G0.txt", "G1_2.txt", "G4_2.txt", "G4_8.txt"]
    meth = tmp_path / "methylome"
    meth.mkdir()
    status = rng.choice([0, 2], size=len(where), p=[0.6, 0.4])
    for k, name in enumerate(names):
        if k:
            flip = rng.random(len(where)) < 0.04 * k
            status = np.where(flip, rng.integers(0, 3, size=len(where)), status)
        rows = []
        for i, ((g, p), s) in enumerate(zip(where, status)):
            post = [0.9999, 0.7][int(rng.integers(10) == 0)]
            line = M.site_line(g["chromosome"], p, "+-*"[g["strand"]].replace("*", "+"), "UIM"[int(s)], post,
                               round(float(0.05 + 0.45 * s + 0.04 * rng.random()), 4))
            f = line.split("\t")
            if i % 97 == 5:
                f[6] = (LONG, "nan", "1e400")[i % 3] if post == 0.9999 else "0.70000000000000000000000"
            if i % 211 == 7 + k:
                f[7] = "XQ"[i % 2]                       # the warning of a device record, or — on a deferred row — of the host
            if i == 40:
                f[6], f[7] = LONG, "Z"
            if i == 41:
                f[8] = "0x1p-1"                          # deferred, and no site for the host
            rows.append("\t".join(f))
        (meth / name).write_text(M.HEADER + "".join(r + "\n" for r in rows))
    nodes = "filename\tnode\tgen\tmeth\n" + "".join(
        f"{meth}/{f}\t{node}\t{gen}\t{m}\n" for f, node, gen, m in
        [("G0.txt", "0_0", 0, "Y"), ("G1_2.txt", "1_2", 1, "Y"), ("G1_8.txt", "1_8", 1, "N"), ("G2_2.txt", "2_2", 2, "N"),
         ("G2_8.txt", "2_8", 2, "N")]) + "-\t3_2\t3\tN\n-\t3_8\t3\tN\n" + f"{meth}/G4_2.txt\t4_2\t4\tY\n{meth}/G4_8.txt\t4_8\t4\tY\n"
    (tmp_path / "nodelist.fn").write_text(nodes)
    (tmp_path / "edgelist.fn").write_text((GOLDEN / "data" / "edgelist.txt").read_text())
    common = ["--methylome", str(meth), "--genome", str(GOLDEN / "annotation.txt"), "--nodes", str(tmp_path / "nodelist.fn"),
              "--edges", str(tmp_path / "edgelist.fn"), "--iterations", "10", "--seed", "77", "-s", "5", "-w", "5", "-c", "2048"]
    got = {}
    for side in ("host", "device"):
        out = tmp_path / f"out_{side}"
        out.mkdir()
        r = subprocess.run([str(B.META_CLI), "-o", str(out), *common, "--sites", side], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        got[side] = ({p.name: p.read_bytes() for p in sorted(out.iterdir())}, r.stdout.replace(str(out), "OUT"), r.stderr)
    a, b = got["host"], got["device"]
    assert sorted(a[0]) == sorted(b[0]) and len(a[0]) >= 9 and len(a[0]["results.txt"].splitlines()) > 50
    for name in a[0]:
        assert a[0][name] == b[0][name], name
    warnings = [l for l in a[1].splitlines() if l.startswith("Warning")]
    assert len(warnings) >= 8 and any("status: Z" in l for l in warnings) and len({l for l in warnings}) >= 3
    assert a[1] == b[1] and a[2] == b[2]                                       # the console: the warnings in file order
    for extra in (["--parse", "host"], ["--genes", "host"]):
        r = subprocess.run([str(B.META_CLI), "-o", str(tmp_path), *common, "--sites", "device", *extra], capture_output=True,
                           text=True, timeout=60)
        assert r.returncode != 0 and "--sites device needs --parse device and --genes device" in r.stderr
    r = subprocess.run([str(B.META_CLI), "-o", str(tmp_path), "--sites", "gpu"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--sites expects host or device" in r.stderr
