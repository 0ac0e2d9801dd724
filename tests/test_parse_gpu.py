"""abn_sites_parse (alphabeta_rs_amd/csrc/abn_parse_kernels.hpp) against the host's parser: every test compares the
device's records record for record and bit for bit with abh_parse_sites (parse_site_full on every line), the deferred
list with what the shared line parser predicts on the CPU, and the host layer's merge of the two (parse_sites_device)
with the host's sequence once more."""
import subprocess

import numpy as np
import pytest

import _parse_model as P

pytestmark = pytest.mark.gpu
GOLDEN = P.ROOT / "tests" / "golden"


@pytest.fixture(scope="module")
def L():
    return P.hostlib()


def check(ctx, L, text, *, skip_lines=1, slab_bytes=0, deferred_extra=(), merged=True):
    """device records == the CPU classifier's, deferred list == its deferred lines (+ deferred_extra: lines beyond the
    staging limit), and what is left after the host has decided the deferred lines == the host's sites.  Returns
    (sites, deferred)."""
    sites, deferred = ctx.parse_sites(text, skip_lines=skip_lines, slab_bytes=slab_bytes)
    cls, want = P.classify(L, text, skip_lines)
    host, n_warnings = P.host_sites(L, text, skip_lines)
    spans = P.line_spans(text)
    assert sites["n_lines"] == len(spans)
    want_deferred = sorted(set((np.flatnonzero(cls == P.DEFER) + skip_lines).tolist()) | set(deferred_extra))
    assert deferred["line"].tolist() == want_deferred
    assert deferred["offset"].tolist() == [spans[l][0] for l in want_deferred]
    assert deferred["length"].tolist() == [spans[l][1] for l in want_deferred]
    extra = np.array([l in set(deferred_extra) for l in want["line"]], dtype=bool)
    keys = [k for k, _ in P.FIELDS] + ["status_flag"]
    P.assert_sites_equal(sites, {k: a[~extra] for k, a in want.items()}, keys)
    if not want_deferred:
        P.assert_sites_equal(sites, host)
        assert int(sites["status_flag"].sum()) == n_warnings
    if merged:
        got, warnings = P.device_sites_merged(L, text, skip_lines, slab_bytes)
        P.assert_sites_equal(got, host)
        assert warnings.count("\n") == n_warnings
    return sites, deferred


@pytest.mark.parametrize("variant", ["whole", "crlf", "no_final_newline"])
def test_bundled_methylomes(gpu_ctx, L, variant):
    for path in P.GOLDEN_METHYLOMES:
        text = path.read_bytes()
        text = {"whole": text, "crlf": text.replace(b"\n", b"\r\n"), "no_final_newline": text.rstrip(b"\n")}[variant]
        for skip in (1, 0):
            sites, deferred = check(gpu_ctx, L, text, skip_lines=skip)
            assert len(sites["line"]) == 500 and len(deferred["line"]) == 0 and sites["kernel_ms"] > 0.0


def test_torture_text(gpu_ctx, L):
    text = P.torture_text()
    for t in (text, text.replace(b"\n", b"\r\n"), text.rstrip(b"\n")):
        sites, deferred = check(gpu_ctx, L, t)
        assert len(deferred["line"]) > 30 and len(sites["line"]) > 100 and int(sites["status_flag"].sum()) >= 6
    got, warnings = P.device_sites_merged(L, text)
    assert "invalid methylation status: X. Parsed as Unmethylated" in warnings


def test_plain_lines_are_never_deferred(gpu_ctx, L):
    """the condition of the issue: at most 15 significant digits and no exponent -> zero lines deferred"""
    sites, deferred = check(gpu_ctx, L, P.plain_text(3000, seed=11))
    assert len(deferred["line"]) == 0 and len(sites["line"]) > 300


@pytest.mark.parametrize("n_lines", [0, 1, P.RUN - 1, P.RUN, P.RUN + 1, 2 * P.RUN + 1])
def test_run_boundaries(gpu_ctx, L, n_lines):
    for final_newline in (True, False):
        text = P.plain_text(n_lines, seed=n_lines, cg_every=2, final_newline=final_newline)
        sites, _ = check(gpu_ctx, L, text)
        check(gpu_ctx, L, text, skip_lines=0, merged=False)
        assert (len(sites["line"]) > 0) == (n_lines > 1) or n_lines == 1


def test_empty_and_header_only(gpu_ctx, L):
    for text in (b"", P.HEADER.encode(), P.HEADER.encode().rstrip(b"\n"), b"\n", b"\n\n", b"\r\n"):
        for skip in (0, 1, 5):
            sites, deferred = check(gpu_ctx, L, text, skip_lines=skip)
            assert len(sites["line"]) == 0 and len(deferred["line"]) == 0
    sites, _ = check(gpu_ctx, L, b"1 2 3 E", skip_lines=0)                 # one line, no header, no line end
    assert sites["start"].tolist() == [2] and sites["strand"].tolist() == [2]


def test_newline_on_both_sides_of_a_piece_boundary(gpu_ctx, L):
    """a '\\n' on the last byte of a 16-byte piece and on the first byte of the next, at several places of a workgroup's
    4 KiB of text"""
    site = P.cg_line(pos="7", tri="CGA").encode()
    for at in (15, 31, 4095, 4111):
        head = b"h" * 15 + b"\n"
        body = b""
        while len(head) + len(body) + len(site) + 1 <= at:
            body += site + b"\n"
        fill = at - (len(head) + len(body))            # a 4-field row that ends right in front of `at`
        row = b"1 2 3 " + b"E" * (fill - 6) if fill >= 7 else b"x" * fill
        text = head + body + row + b"\n\n" + site + b"\n" if at > 15 else head + b"\n" + site + b"\n"
        assert text[at] == 10 and text[at + 1] == 10 and at % 16 == 15
        sites, _ = check(gpu_ctx, L, text)
        assert len(sites["line"]) >= 1


def test_staging_limit(gpu_ctx, L):
    """a line one byte below, at, and one byte above what the stage holds (the line's offset in its first 16-byte piece
    counts); the run's other lines are parsed around it"""
    short = [P.cg_line(pos=str(i), tri="CGA") for i in range(40)]
    for over in (-1, 0, 1, 5000):
        head = (P.HEADER + "\n".join(short[:20]) + "\n").encode()
        length = P.STAGE - len(head) % 16 + over
        long_line = b"1 2 3 " + b"E" * (length - 6)
        text = head + long_line + b"\n" + ("\n".join(short[20:]) + "\n").encode()
        sites, deferred = check(gpu_ctx, L, text, deferred_extra=[21] if over > 0 else [])
        assert len(deferred["line"]) == (1 if over > 0 else 0) and len(sites["line"]) == (40 if over > 0 else 41)
    # ... with a '\r' in front of the line end: not part of the deferred line's length
    text = head + long_line + b"\r\n"
    _, deferred = check(gpu_ctx, L, text, deferred_extra=[21])
    assert deferred["length"].tolist() == [len(long_line)]


def test_slabs(gpu_ctx, L):
    """a 2000-line text in slabs small enough for at least three, one nominal boundary directly behind a '\\n' and one
    that falls inside a line; the same records as in one slab"""
    text = P.plain_text(2000, seed=3, cg_every=3)
    spans = P.line_spans(text)
    slab = spans[600][0]                                # the first slab's nominal end is the begin of line 600
    assert text[slab - 1] == 10 and text[2 * slab - 1] != 10 and len(text) > 2 * slab
    whole, _ = check(gpu_ctx, L, text)
    for s in (slab, slab + 1, 4096):
        sites, _ = check(gpu_ctx, L, text, slab_bytes=s)
        P.assert_sites_equal(sites, whole)
    check(gpu_ctx, L, P.plain_text(150, seed=4, cg_every=3), slab_bytes=1)      # every line is longer than the slab
    torture = P.torture_text()
    one, d1 = gpu_ctx.parse_sites(torture)
    many, d2 = check(gpu_ctx, L, torture, slab_bytes=700)
    P.assert_sites_equal(many, one)
    assert all(np.array_equal(d1[k], d2[k]) for k in d1)


def outputs(directory):
    return {p.name: p.read_bytes() for p in sorted(directory.iterdir()) if p.is_file()}


def test_alphabeta_cli_parses_on_either_side(tmp_path):
    """`alphabeta -n -e` on the bundled nodelist: every output file and the console byte-identical under --parse"""
    from alphabeta_rs_amd import build as B

    B.build_host()
    got = {}
    for where in ("host", "device"):
        out = tmp_path / where
        out.mkdir()
        r = subprocess.run([str(B.CLI), "-i", "50", "-n", "./data/nodelist.txt", "-e", "./data/edgelist.txt", "-o", str(out),
                            "--parse", where], capture_output=True, text=True, timeout=300, cwd=str(GOLDEN))
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        got[where] = (outputs(out), r.stdout.replace(str(out), "OUT"))
    assert set(got["host"][0]) >= {"pedigree.txt", "analysis.txt", "raw.npy"}
    assert got["host"] == got["device"]
    r = subprocess.run([str(B.CLI), "--parse", "gpu"], capture_output=True, text=True, timeout=60, cwd=str(GOLDEN))
    assert r.returncode == 2 and "--parse expects host or device" in r.stderr


def test_metaprofile_cli_parses_on_either_side(tmp_path):
    """`metaprofile_alphabeta --methylome` on methylomes laid over the bundled annotation's genes (CG rows among rows of
    other contexts, a row with an invalid status): every output file and the console byte-identical under --parse"""
    from alphabeta_rs_amd import build as B

    import _windows_model as M

    B.build_host()
    _, genes = M.genome_of((GOLDEN / "annotation.txt").read_text())
    rng = np.random.default_rng(8)
    where = []
    for g in sorted(genes, key=lambda g: (g["chromosome"], g["start"]))[:3]:
        where += [(g, int(p)) for p in sorted(rng.integers(g["start"] - 2100, g["end"] + 2100, size=1000))]
    meth = tmp_path / "methylome"
    meth.mkdir()
    names = ["G0.txt", "G1_2.txt", "G4_2.txt", "G4_8.txt"]
    status = rng.choice([0, 2], size=len(where), p=[0.6, 0.4])
    for k, name in enumerate(names):
        flip = rng.random(len(where)) < 0.04 * k
        status = np.where(flip, rng.integers(0, 3, size=len(where)), status)
        rows = []
        for i, ((g, p), s) in enumerate(zip(where, status)):
            strand = "+-*"[g["strand"]].replace("*", "+")
            level = f"{0.05 + 0.45 * s + 0.04 * rng.random():.4f}"
            rows.append(P.cg_line(str(g["chromosome"]), str(p), strand, "CG", "3", "8", "0.9999", "UIM"[int(s)], level, "CGA"))
            rows.append(P.cg_line(str(g["chromosome"]), str(p + 1), strand, "CHH", "0", "8", "0.7000", "U", "0.0100", "CCA"))
            if i == 17:
                rows[-2] = P.cg_line(str(g["chromosome"]), str(p), strand, "CG", "3", "8", "0.9999", "X", level, "CGA")
        (meth / name).write_text(P.HEADER + "\n".join(rows) + "\n")
    nodes = "filename\tnode\tgen\tmeth\n" + "".join(
        f"{meth}/{f}\t{node}\t{gen}\t{m}\n" for f, node, gen, m in
        [("G0.txt", "0_0", 0, "Y"), ("G1_2.txt", "1_2", 1, "Y"), ("G1_8.txt", "1_8", 1, "N"), ("G2_2.txt", "2_2", 2, "N"),
         ("G2_8.txt", "2_8", 2, "N")]) + "-\t3_2\t3\tN\n-\t3_8\t3\tN\n" + f"{meth}/G4_2.txt\t4_2\t4\tY\n{meth}/G4_8.txt\t4_8\t4\tY\n"
    (tmp_path / "nodelist.fn").write_text(nodes)
    (tmp_path / "edgelist.fn").write_text((GOLDEN / "data" / "edgelist.txt").read_text())
    got = {}
    for side in ("host", "device"):
        out = tmp_path / side
        out.mkdir()
        r = subprocess.run([str(B.META_CLI), "-o", str(out), "--methylome", str(meth), "--genome", str(GOLDEN / "annotation.txt"),
                            "--nodes", str(tmp_path / "nodelist.fn"), "--edges", str(tmp_path / "edgelist.fn"), "--iterations",
                            "20", "--seed", "77", "-s", "5", "-w", "5", "-c", "2048", "--parse", side],
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        got[side] = (outputs(out), sorted(r.stdout.splitlines()))   # (the host's threads print the warnings in any order)
    assert {"results.txt", "raw.npy"} <= set(got["host"][0]) and len(got["host"][0]["results.txt"].splitlines()) > 50
    assert got["host"][1].count("Warning: Encountered invalid methylation status: X. Parsed as Unmethylated") == 4
    assert got["host"] == got["device"]
