"""The pedigree build from resident sites (abn_codes_*, alphabeta_rs_amd/csrc/abn_codes.hpp) against the host forms: the
packed matrix byte for byte against abn_pack_codes of the host's code bytes, the rc_meth_lvl folds against a Python float
loop, the pairwise result against the scan of the host matrix, and `alphabeta --sites device` file for file against
`--sites host`."""
import ctypes as C
import os
import shutil
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

import _codes_model as K
import _parse_model as P
from test_sites_resident_gpu import LONG, Deferring, decide, slabs

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden"
FLT = K.FILTER
INVALID = 1  # ABN_ERR_INVALID_ARG
SITE_COUNTS = (0, 1, 15, 16, 17, 255, 256, 257, 1025, 2755)


@pytest.fixture(scope="module")
def L():
    return P.hostlib()


def methylome(n_sites, seed, pm=None):
    """a methylome text of exactly n_sites CG rows among rows of other contexts (no site), posteriors on both sides of the
    filter and at it, levels of -0.0 among the others"""
    rng = np.random.default_rng(seed)
    rows = []
    for i in range(n_sites):
        while rng.integers(4) == 0:
            rows.append(P.cg_line(pos=str(len(rows) + 1), ctx=("CHH", "CHG")[int(rng.integers(2))], tri="CCT"))
        post = pm or ("0.9999", "0.99", f"{rng.random():.4f}", "0.5")[int(rng.integers(4))]
        level = "-0.0" if rng.integers(5) == 0 else f"{rng.random():.4f}"
        rows.append(P.cg_line(pos=str(len(rows) + 1), strand="+-"[int(rng.integers(2))], pm=post, st="UIM"[int(rng.integers(3))],
                              ml=level, tri="CGA"))
    return P.HEADER + "".join(r + "\n" for r in rows)


def resident(ctx, L, text, slab_bytes):
    """Context.parse_sites_resident as the pedigree build reads a file (every line, src/pedigree.rs:147-163) with the
    host-decided lines inserted"""
    r = ctx.parse_sites_resident(text, skip_lines=0, slab_bytes=slab_bytes)
    r.insert(*decide(L, text, r.deferred()))
    return r


def host_forms(abn, L, texts, slab_bytes):
    """from the merged host sequences (P.device_sites_merged): (site counts, packed rows, [(sum bytes, kept)])"""
    merged = [P.device_sites_merged(L, t, 0, slab_bytes)[0] for t in texts]
    codes = [K.code_bytes(m["status"], m["posteriormax"]) for m in merged]
    return merged, [len(c) for c in codes], K.packed_rows(abn, codes), [K.fold(m["posteriormax"], m["meth_lvl"]) for m in merged]


def assert_stats(codes, counts, folds):
    count, lsk, kept = codes.stats()
    assert count.dtype == kept.dtype == np.int64 and lsk.dtype == np.float64
    assert count.tolist() == counts and kept.tolist() == [k for _, k in folds]
    assert [struct.pack("<d", v) for v in lsk] == [s for s, _ in folds]


@pytest.mark.parametrize("slab_bytes", [0, 4096, 300])
def test_codes_from_parsed_equals_host_forms(abn, gpu_ctx, L, slab_bytes):
    first = last = adjacent = whole = nan_inserted = neg0_counted = 0
    for case, n_sites in enumerate(SITE_COUNTS):
        n_samples = 2 + case % 3
        samples = [Deferring(methylome(n_sites, 100 * case + s)) for s in range(n_samples)]
        for s, d in enumerate(samples):
            d.slab = slab_bytes or 1 << 26                                           # (0: the whole text is one slab)
            n = len(d.lines)
            if s == 1 and n_sites >= 15:
                d.whole = all([d.mark(i) for i in range(1, n) if "\tCG\t" in d.lines[i]])   # every site of one sample
                continue
            d.whole = False
            for chunk in (0, 1, 2):
                d.mark_chunk_edges(chunk)
            if n > 40:
                d.mark(n // 2), d.mark(n // 2 + 1), d.mark(n // 2 + 2)
        texts = [d.text() for d in samples]
        merged, counts, want_packed, folds = host_forms(abn, L, texts, slab_bytes)
        assert counts == [n_sites] * n_samples, case                               # a marked row stays a site for the host
        n_inserted = 0
        for d, m, t in zip(samples, merged, texts):                                # the marks that hit a site, by where
            hit = d.marked & set(m["line"].tolist())
            n_inserted += len(hit)
            whole += d.whole and len(hit) == n_sites
            if not d.whole:
                cut = slabs(t, d.slab)
                first += sum(a in hit for a, _ in cut)
                last += sum(b in hit for _, b in cut)
                adjacent += sum(l + 1 in hit for l in hit)
        sites = [resident(gpu_ctx, L, t, slab_bytes) for t in texts]
        codes = abn.Codes.from_parsed(gpu_ctx, sites, posterior_max_filter=FLT)
        try:
            assert sum(s.info()["n_deferred"] for s in sites) >= n_inserted
            stride = max(abn.packed_row_stride(n_sites), 64)
            assert codes.info() == {"n_samples": n_samples, "n_sites": n_sites, "row_stride": stride, "same_len": True}
            got = codes.packed()
            assert got.shape == want_packed.shape and got.tobytes() == want_packed.tobytes(), case   # padding included
            assert_stats(codes, counts, folds)
            want_pairs = gpu_ctx.pairwise_divergence_packed(want_packed, n_sites)
            for x, y in zip(codes.pairwise(), want_pairs):
                assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), case
            assert codes.packed_device_ptr() % 16 == 0 and codes.packed_device_ptr() != 0
            ms = codes.kernel_ms()
            assert ms.shape == (4,) and np.all(ms >= 0), (case, ms)
            if 0 < n_inserted < n_sites * n_samples:                                # inserted lines, and device records
                assert np.all(ms > 0), (case, ms)
            again = abn.Codes.from_parsed(gpu_ctx, sites, posterior_max_filter=FLT)     # the handles are not consumed
            assert again.packed().tobytes() == got.tobytes()
            assert_stats(again, counts, folds)
            again.close()
            for m in merged:
                nan_inserted += int(np.isnan(m["posteriormax"]).sum())
                neg0_counted += int((np.signbit(m["meth_lvl"]) & K.counted(m["posteriormax"])).sum())
        finally:
            codes.close()
            for s in sites:
                s.close()
    # (the one slab of slab_bytes 0 begins with the header row, which is no site)
    assert (first >= 5 or slab_bytes == 0) and last >= 5 and adjacent >= 10 and whole == 8, (first, last, adjacent, whole)
    assert nan_inserted > 100 and neg0_counted > 100, (nan_inserted, neg0_counted)


def test_further_cases(abn, gpu_ctx, L):
    """a `nan` posterior row, an all-filtered sample, zero sites in all samples, one sample only, samples of different length"""
    rows = [P.cg_line(pos="5", pm="0.9999", ml="0.25"), P.cg_line(pos="6", pm="nan", st="M", ml="0.5"),
            P.cg_line(pos="7", pm="0.2", ml="0.125"), P.cg_line(pos="8", pm=LONG, st="I", ml="-0.0")]
    nan_text = (P.HEADER + "".join(r + "\n" for r in rows)).encode()
    filtered = methylome(300, 5, pm="0.5").encode()
    plain = methylome(300, 6).encode()
    empty = P.HEADER.encode()
    for name, texts in (("nan", [nan_text, nan_text]), ("all filtered", [plain, filtered, plain]), ("no sites", [empty, b"", empty]),
                        ("one sample", [plain]), ("one empty sample", [b""]), ("ragged", [plain, methylome(299, 7).encode(), empty])):
        merged, counts, want_packed, folds = host_forms(abn, L, texts, 300)
        sites = [resident(gpu_ctx, L, t, 300) for t in texts]
        codes = abn.Codes.from_parsed(gpu_ctx, sites, posterior_max_filter=FLT)
        try:
            same = len(set(counts)) == 1
            assert codes.info() == {"n_samples": len(texts), "n_sites": max(counts), "same_len": same,
                                    "row_stride": max(abn.packed_row_stride(max(counts)), 64)}, name
            assert codes.packed().tobytes() == want_packed.tobytes(), name
            assert_stats(codes, counts, folds)
            if same:
                want = gpu_ctx.pairwise_divergence_packed(want_packed, counts[0])
                got = codes.pairwise()
                assert all(x.tobytes() == y.tobytes() and x.shape == (len(texts) * (len(texts) - 1) // 2,) for x, y in zip(got, want)), name
            else:
                with pytest.raises(abn.AbnError) as e:                              # refused, and the text says why
                    codes.pairwise()
                assert e.value.status == INVALID and "differ in length" in str(e.value)
                assert_stats(codes, counts, folds)                                  # the stats stay valid
            if name == "nan":
                assert counts == [4, 4] and folds[0] == (struct.pack("<d", 0.25 + -0.0), 2)
                assert codes.packed()[0, :4].tolist() == [0xfc | 2, 0xfc | 2, 0xff, 0xfc | 1]       # NaN (site 1): not filtered
            if name == "all filtered":
                assert folds[1] == (struct.pack("<d", 0.0), 0) and codes.stats()[2].tolist()[1] == 0
                assert set(codes.packed()[1].tolist()) == {0xff}
            if name == "no sites":
                assert counts == [0, 0, 0] and codes.row_stride == 64 and set(codes.packed().ravel().tolist()) == {0xff}
        finally:
            codes.close()
            for s in sites:
                s.close()
    # fewer than two samples: ABN_OK, nothing written
    one = resident(gpu_ctx, L, plain, 0)
    codes = abn.Codes.from_parsed(gpu_ctx, [one], posterior_max_filter=FLT)
    d = np.full(1, 7, dtype=np.uint64)
    assert gpu_ctx._L.abn_codes_pairwise(codes._h, d.ctypes.data_as(C.POINTER(C.c_uint64)), None, None) == 0 and d[0] == 7
    codes.close()
    one.close()


def test_bad_arguments(abn, gpu_ctx, L):
    """every ABN_ERR_INVALID_ARG case of abn_codes_create_parsed is a status code, and no handle comes back"""
    lib = gpu_ctx._L
    text = (P.HEADER + "\n".join([P.cg_line(pos="5"), P.cg_line(pos="6", pm=LONG), P.cg_line(pos="7")]) + "\n").encode()

    def create(handles, ctx=gpu_ctx, n=None, out=True, samples=True):
        raw = [h._h if hasattr(h, "_h") else h for h in handles]
        arr = (C.c_void_p * max(len(raw), 1))(*(h.value if isinstance(h, C.c_void_p) else h for h in raw))
        w = C.c_void_p(0xdead)
        rc = lib.abn_codes_create_parsed(ctx._h if ctx else None, FLT, len(handles) if n is None else n, arr if samples else None,
                                         C.byref(w) if out else None)
        if rc and ctx and out:
            assert not w.value
        return rc, w

    r = gpu_ctx.parse_sites_resident(text, skip_lines=0)
    assert r.info()["n_deferred"] == 1
    assert create([r])[0] == INVALID                                               # the forgotten insert
    r.insert(*decide(L, text, r.deferred()))
    rc, w = create([r])
    assert rc == 0 and w.value and lib.abn_codes_destroy(w) == 0
    assert create([r], ctx=None)[0] == INVALID and create([r], out=False)[0] == INVALID and create([r], samples=False)[0] == INVALID
    assert create([], n=0)[0] == INVALID and create([r], n=-1)[0] == INVALID and create([r], n=65536)[0] == INVALID
    assert create([r, None])[0] == INVALID                                         # a null sample handle
    h = C.c_void_p()
    assert lib.abn_sites_parse(gpu_ctx._h, text, len(text), None, C.byref(h)) == 0
    assert create([h])[0] == INVALID and create([r, h])[0] == INVALID               # a host-form handle
    lib.abn_sites_destroy(h)
    other = abn.Context(0)
    try:
        foreign = other.parse_sites_resident(P.plain_text(20, seed=1), skip_lines=0)
        assert create([foreign])[0] == INVALID and create([r, foreign])[0] == INVALID   # a sites handle of another context
        assert create([r], ctx=other)[0] == INVALID
        foreign.close()
    finally:
        other.close()
    for entry, args in ((lib.abn_codes_destroy, ()), (lib.abn_codes_info, (None,) * 4), (lib.abn_codes_stats, (None,) * 3),
                        (lib.abn_codes_packed, (None,)), (lib.abn_codes_packed_device_ptr, (None,)),
                        (lib.abn_codes_pairwise, (None,) * 3), (lib.abn_codes_kernel_ms, (None,))):
        assert entry(None, *args) == INVALID
    rc, w = create([r])
    assert rc == 0 and lib.abn_codes_packed(w, None) == INVALID and lib.abn_codes_kernel_ms(w, None) == INVALID
    lib.abn_codes_destroy(w)
    r.close()


# ---------------------------------------------------------------- the host layer and the tool
def outputs(out: Path):
    return {p.name: p.read_bytes() for p in sorted(out.iterdir())}


def run_tool(tmp_path, nodes, edges, cwd):
    """`alphabeta` with --sites host and --sites device -> {side: (files, stdout, stderr)}"""
    from alphabeta_rs_amd import build as B

    B.build_host()
    got = {}
    for side in ("host", "device"):
        out = tmp_path / f"out_{side}"
        out.mkdir()
        r = subprocess.run([str(B.CLI), "-i", "50", "-n", str(nodes), "-e", str(edges), "-o", str(out), "--parse", "device",
                            "--sites", side], capture_output=True, text=True, timeout=300, cwd=str(cwd))
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        got[side] = (outputs(out), r.stdout.replace(str(out), "OUT"), r.stderr)
    a, b = got["host"], got["device"]
    assert set(a[0]) >= {"pedigree.txt", "analysis.txt", "raw.npy"} and sorted(a[0]) == sorted(b[0])
    for name in a[0]:
        assert a[0][name] == b[0][name], name
    assert a[1] == b[1] and a[2] == b[2]
    return got


def doctored_copy(tmp_path, edit):
    """the bundled nodelist, edgelist and methylomes under tmp_path, every methylome's lines through edit(file index, lines)"""
    meth = tmp_path / "methylome"
    meth.mkdir()
    for k, src in enumerate(sorted((GOLDEN / "data" / "methylome").glob("*.txt"))):
        lines = src.read_text().split("\n")[:-1]
        (meth / src.name).write_text("".join(l + "\n" for l in edit(k, lines)))
    nodes = (GOLDEN / "data" / "nodelist.txt").read_text().replace("./data/methylome/", f"{meth}/")
    (tmp_path / "nodelist.txt").write_text(nodes)
    shutil.copy(GOLDEN / "data" / "edgelist.txt", tmp_path / "edgelist.txt")
    return tmp_path / "nodelist.txt", tmp_path / "edgelist.txt"


def test_alphabeta_sites_device_on_the_bundled_data(tmp_path):
    from alphabeta_rs_amd import build as B

    got = run_tool(tmp_path, "./data/nodelist.txt", "./data/edgelist.txt", GOLDEN)
    assert got["device"][0]["pedigree.txt"] == (GOLDEN / "pedigree_generated.txt").read_bytes()
    r = subprocess.run([str(B.CLI), "-n", "./data/nodelist.txt", "-e", "./data/edgelist.txt", "-o", str(tmp_path), "--sites",
                        "device", "--parse", "host"], capture_output=True, text=True, timeout=60, cwd=str(GOLDEN))
    assert r.returncode == 2 and "--sites device needs --parse device" in r.stderr
    r = subprocess.run([str(B.CLI), "--sites", "gpu"], capture_output=True, text=True, timeout=60, cwd=str(GOLDEN))
    assert r.returncode == 2 and "--sites expects host or device" in r.stderr


def test_alphabeta_sites_device_on_a_doctored_copy(tmp_path):
    """rows the device defers, of both outcomes and the same in every file (the samples keep one length), rows with an
    invalid status byte, and one `0x1p-1` row"""
    seen = {"deferred": 0, "status": 0, "hex": 0}

    def edit(k, lines):
        cg = [i for i, l in enumerate(lines) if l.split("\t")[3:4] == ["CG"]]
        for j, i in enumerate(cg):
            f = lines[i].split("\t")
            if j % 41 == 3:
                f[6] = (LONG, "nan", "1e400", "abc")[(j // 41) % 4]                 # accepted thrice, then no site
                seen["deferred"] += 1
            if j % 97 == 5 + k:
                f[7] = "XQ"[j % 2]                                                  # a device record's warning
                seen["status"] += 1
            if j == 40:
                f[6], f[7] = LONG, "Z"                                              # ... and the host's, on a deferred row
            if j == 50:
                f[8] = "0x1p-1"                                                     # deferred, and no site for the host
                seen["hex"] += 1
            lines[i] = "\t".join(f)
        return lines

    nodes, edges = doctored_copy(tmp_path, edit)
    got = run_tool(tmp_path, nodes, edges, tmp_path)
    assert seen["deferred"] >= 40 and seen["status"] >= 8 and seen["hex"] == 4
    warnings = [l for l in got["device"][1].splitlines() if l.startswith("Warning")]
    assert len(warnings) >= 12 and any("status: Z" in l for l in warnings) and len(set(warnings)) >= 3
    assert "Lengths do not match" not in got["device"][1]
    assert got["device"][0]["pedigree.txt"] != (GOLDEN / "pedigree_generated.txt").read_bytes()


def test_alphabeta_sites_device_with_a_methylome_a_site_short(tmp_path):
    def edit(k, lines):
        if k == 2:
            del lines[[i for i, l in enumerate(lines) if l.split("\t")[3:4] == ["CG"]][7]]
        return lines

    nodes, edges = doctored_copy(tmp_path, edit)
    got = run_tool(tmp_path, nodes, edges, tmp_path)
    assert got["device"][1].count("Lengths do not match, all bets are off") == 3     # the pairs with the short sample


def test_resident_build_counter_and_result(tmp_path):
    """Pedigree::build with --sites device, in process: the rows and p0uu of the packed-entry build, and the counter of
    resident builds rises by one"""
    from alphabeta_rs_amd import build as B

    B.build_host()
    H = C.CDLL(str(B.PEDIGREE_LIB))
    sig = [C.c_char_p, C.c_char_p, C.c_double, C.c_char_p, C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_double), C.c_char_p, C.c_int]
    H.abh_pedigree_build_gpu.argtypes = H.abh_pedigree_build_resident.argtypes = sig
    H.abh_resident_build_calls.restype = H.abh_packed_scan_calls.restype = C.c_longlong
    before, scans = H.abh_resident_build_calls(), H.abh_packed_scan_calls()
    res = {}
    cwd = os.getcwd()
    os.chdir(GOLDEN)  # the nodelist names ./data/methylome/*.txt relative to the working directory
    try:
        for name, entry in (("host", H.abh_pedigree_build_gpu), ("device", H.abh_pedigree_build_resident)):
            rows, p0, err = np.zeros((64, 4)), C.c_double(), C.create_string_buffer(256)
            out = tmp_path / f"{name}.txt"
            n = entry(b"./data/nodelist.txt", b"./data/edgelist.txt", 0.99, str(out).encode(),
                      rows.ctypes.data_as(C.POINTER(C.c_double)), 64, C.byref(p0), err, 256)
            assert n == 6, err.value
            res[name] = (rows[:n].tobytes(), struct.pack("<d", p0.value), out.read_bytes())
    finally:
        os.chdir(cwd)
    assert res["host"] == res["device"]
    assert res["device"][2] == (GOLDEN / "pedigree_generated.txt").read_bytes()
    assert H.abh_resident_build_calls() == before + 1 and H.abh_packed_scan_calls() == scans + 1   # (the host side's scan)
