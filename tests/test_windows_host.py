"""The host half of the window extraction (alphabeta_rs_amd/host/windows_extract.hpp) against the Python restatement of the
reference in tests/_windows_model.py: the annotation parser and its gene lists, the gene choice of every site with the
last_gene cache, Windows::new's counts — and the parsers once more under the host sanitizers, in a stand-alone program.
No GPU."""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import _windows_model as M

ROOT = Path(__file__).resolve().parent.parent
ANNOTATION = (ROOT / "tests" / "golden" / "annotation.txt").read_text()

HAND_WRITTEN = "\n".join([
    "seqnames\tstart\tend\twidth\tstrand\tgbM.id",                # a header: no strand anywhere
    "1\t6362000\t6362200\t201\t*\tAT1G18480",                     # second format, '*' strand
    "chr2 500 900 401 - SECOND_MINUS",                            # second format, spaces, chr prefix
    "chrchr3\t10\t20\tNAME\tanno\t+",                             # first format, the prefix twice
    "chrM\t5\t50\tMITO\tanno\t-",
    "C\t7\t70\tCHLORO\tanno\t*",
    "1\t900\t800\tBACKWARDS\tanno\t+",                            # end < start: kept, its length wraps
    "1\t100\t200\tBADSTRAND\tanno\t?",                            # bad strand in both places
    "1\t100\t200\t+\tanno\tx",                                    # strand only where neither format has it
    "1\tabc\t200\tBADSTART\tanno\t+",                             # first format by its strand, then a parse error: dropped
    "1\t300\t400\t5\t+\t-",                                       # both strands correct: the first format wins
    "300\t1\t2\tBADCHROM\tanno\t+",                               # 300 is no u8
    "1\t4294967296\t5\tOVERFLOW\tanno\t+",
    "1\t+40\t60\tPLUS\tanno\t-",                                  # Rust parses "+40"
    "1\t50\t60\tSEVEN\tanno\t+\textra",
    "",
    "1\t20\t90\tUNSORTED_EARLY\tanno\t+",                         # unsorted input, and equal starts keep input order
    "1\t20\t70\tUNSORTED_TWIN\tanno\t+",
]) + "\n"


def model_lists(text):
    genome, genes = M.genome_of(text)
    s = ""
    for c in sorted(genome):
        for tag, key in (("s", "sense"), ("a", "antisense"), ("c", "combined")):
            for g in genome[c][key]:
                s += f"{c} {tag} {g['start']} {g['end']} {g['strand']} {g['name']}\n"
    return s, len(genes), (M.max_gene_length(genes, True) if genes else 0)


def host_lists(L, text):
    import ctypes as C

    t = text.encode()
    out, out2 = C.create_string_buffer(1 << 20), (C.c_longlong * 2)()
    n = L.abh_annotation_lists(t, len(t), out, 1 << 20, out2)
    assert n >= 0
    return out.value.decode(), out2[0], out2[1]


def test_annotation_parse_and_gene_lists_equal_the_model():
    L = M.hostlib()
    for text in (ANNOTATION, HAND_WRITTEN, ANNOTATION + HAND_WRITTEN, HAND_WRITTEN.replace("\n", "\r\n"), ""):
        assert host_lists(L, text) == model_lists(text)
    lists, n, mgl = host_lists(L, ANNOTATION)
    assert n == 100 and mgl > 0
    lists, n, mgl = host_lists(L, HAND_WRITTEN)
    assert n == 10 and mgl == (800 - 900) % 2**32                 # the reference's release build wraps here too
    assert "1 s 20 90 0 UNSORTED_EARLY\n1 s 20 70 0 UNSORTED_TWIN\n" in lists     # stable
    assert "BADSTART" not in lists and "1 a 300 400 1 5\n" in lists


def site(chrom, pos, strand="+", status="M", post=0.9999, level=0.5):
    return M.site_line(chrom, pos, strand, status, post, level)


def choice_equal(L, annotation, lines, args):
    text = "header\n" + "\n".join(lines) + "\n"
    genome, _ = M.genome_of(annotation)
    pairs = M.choose_genes(text, genome, args)
    want = M.soa([pairs], args)[1:]
    got = M.host_choose_genes(L, annotation, text, args)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and np.array_equal(g, w)
    return pairs


def test_gene_choice_equals_the_model():
    L = M.hostlib()
    # two sense genes whose flanks overlap at cutoff 100 (A ends 1200, B starts 1300), an antisense gene between them, a
    # '*' gene on chromosome 2, a nested pair on chromosome 3 (the search key end + cutoff is not sorted there)
    ann = "\n".join(["1\t1000\t1200\tA\tx\t+", "1\t1300\t1500\tB\tx\t+", "1\t1100\t1400\tANTI\tx\t-",
                     "2\t500\t700\tSTAR\tx\t*", "3\t100\t5000\tOUTER\tx\t+", "3\t200\t300\tINNER\tx\t+",
                     "3\t6000\t6100\tLATER\tx\t+"]) + "\n"
    args = M.Args(cutoff=100, step=5, size=5)
    lines = [site(1, p) for p in (898, 899, 900, 901, 1199, 1200, 1201)]                    # gene.start - cutoff, gene.end
    lines += [site(1, p) for p in (1210, 1250, 1299, 1300, 1301, 1310)]                      # the overlap: A is kept
    lines += [site(1, p) for p in (1598, 1599, 1600, 1601)]                                  # B.end + cutoff (end = start + 1)
    lines += [site(1, 1250, "-"), site(1, 1250), site(1, 1501, "-"), site(1, 999, "-")]      # strand switches drop the cache
    lines += [site(7, 1250), site("chrM", 10), site("X", 10)]                               # no such chromosome; no chromosome
    lines += [f"2\t{p}\t{p + 3}\tE10" for p in (390, 400, 650, 797, 798, 800, 801)]          # unknown strand: 4-field rows
    lines += [site(2, 600, "-"), site(2, 600, "+")]                                         # '*' gene equals both strands
    lines += [f"1\t1005\t1007\tCG\tx\t+\t3\t8\t0.5\tI\t0.25"]                                # third format, filtered
    lines += [site(3, p) for p in (150, 250, 350, 400, 5050, 5100, 5101, 5950, 6000, 6200, 6201)]
    lines += ["1\t1000\t+\tCHH\t0\t8\t0.9\tU\t0.1", "garbage", "", "1\t1000\t+\tCG\t0\t8\t0.9\t\t0.1"]
    pairs = choice_equal(L, ann, lines, args)
    by_pos = {(s["chromosome"], s["start"], s["strand"]): (g or {}).get("name") for s, g in pairs}
    assert by_pos[(1, 899, 0)] is None and by_pos[(1, 900, 0)] == "A"                        # start + cutoff >= gene.start
    # 1300: the search stops on A (its key end + cutoff IS 1300), and the site's end 1301 is beyond A's flank: no gene
    assert by_pos[(1, 1299, 0)] == "A" and by_pos[(1, 1300, 0)] is None and by_pos[(1, 1301, 0)] == "B"
    assert by_pos[(1, 1599, 0)] == "B" and by_pos[(1, 1600, 0)] is None
    assert by_pos[(2, 400, 2)] == "STAR" and by_pos[(2, 390, 2)] is None and by_pos[(7, 1250, 0)] is None
    assert len(pairs) == len(lines) - 5                                                      # "X", CHH, garbage, "", no status
    # cutoff_gene_length: every gene brings a flank of its own length
    choice_equal(L, ann, lines, M.Args(cutoff=100, step=5, size=5, cutoff_gene_length=True))
    # and the whole annotation with sites around every gene, cache and search together
    genome, genes = M.genome_of(ANNOTATION)
    rng = np.random.default_rng(7)
    for a in (M.Args(cutoff=2048), M.Args(cutoff=300, cutoff_gene_length=True)):
        lines = []
        for g in sorted(genes, key=lambda g: (g["chromosome"], g["start"])):
            for p in sorted(rng.integers(max(g["start"] - 2100, 0), g["end"] + 2100, size=12)):
                lines.append(site(g["chromosome"], int(p), "+-"[int(rng.integers(2))]))
        pairs = choice_equal(L, ANNOTATION, lines, a)
        assert 0 < sum(g is not None for _, g in pairs) < len(pairs)


def test_window_counts_are_windows_new():
    import ctypes as C

    L = M.hostlib()
    out = (C.c_int * 3)()
    for cutoff, step, size, absolute, mgl in [(2048, 5, 5, 0, 100), (2048, 3, 5, 0, 100), (2048, 256, 512, 1, 4096),
                                              (20, 7, 7, 1, 40), (2048, 1, 5, 0, 100), (10, 30, 30, 1, 29)]:
        L.abh_window_counts(cutoff, step, size, absolute, mgl, out)
        assert tuple(out) == M.windows_new(M.Args(cutoff, step, size, bool(absolute)), mgl)


def test_host_parsers_under_address_and_ub_sanitizers(tmp_path):
    """A stand-alone program (its own main, run directly): truncated and corrupted annotation and methylome text through
    the new host parsers, built with -fsanitize=address,undefined."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not found")
    exe = tmp_path / "windows_parsers_main"
    r = subprocess.run([gxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                        "-fno-omit-frame-pointer", "-pthread", "-I", str(ROOT / "include"), "-o", str(exe),
                        str(ROOT / "tests" / "native" / "windows_parsers_main.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe), str(ROOT / "tests" / "golden" / "annotation.txt")], capture_output=True, text=True,
                       env={"UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1", "ASAN_OPTIONS": "abort_on_error=1"},
                       timeout=600)
    assert r.returncode == 0 and "sanitized windows ok 400" in r.stdout, r.stdout[-1500:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
