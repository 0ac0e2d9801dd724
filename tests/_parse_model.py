"""What the parser tests share (tests/test_parse_cpu.py, tests/test_parse_gpu.py): the host shims of host_capi.cpp around
the host's line parser (parse_site_full) and the one the device shares (csrc/abn_parse.hpp), the f64 tokens the issue
names with the outcome each must have, and the generated methylome texts."""
import ctypes as C
import struct
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
GOLDEN_METHYLOMES = sorted((ROOT / "tests" / "golden" / "data" / "methylome").glob("*.txt"))
HEADER = ("seqnames\tstart\tstrand\tcontext\tcounts.methylated\tcounts.total\tposteriorMax\tstatus\trc.meth.lvl\t"
          "context.trinucleotide\n")
VALUE, REJECT, DEFER = 0, 1, 2
STAGE = 16384  # kParseStageBytes
RUN = 256      # kParseRun

# token -> the outcome abn_parse_f64 must have.  VALUE: certain, bit-equal to float(); REJECT: strtod takes a proper
# prefix at most; DEFER: one of the kinds the device leaves to the host (the reason beside it)
TOKENS = {
    "1": VALUE, "1.": VALUE, ".5": VALUE, "-0.0": VALUE, "+2.5": VALUE, "1e-3": VALUE, "1E5": VALUE, "0": VALUE,
    "0.9999": VALUE, "0.0493": VALUE, "007.250": VALUE, "-.5e+1": VALUE,
    "0.123456789012345": VALUE,                 # 15 digits
    "0.1234567890123456": VALUE,                # 16 digits, below 2^53
    "0.9999999999999999": DEFER,                # 16 digits, above 2^53
    "0.12345678901234567": DEFER,               # 17 digits: above 2^53
    "1234567890123456789": DEFER,               # 19 digits: above 2^53
    "0.0000000001234567890123456": DEFER,       # 16 digits, q = -25
    "12345678901234567890": DEFER,              # 20 digits
    "0.00000000000000000001": VALUE,            # one digit behind 19 zeros: q = -20
    "9007199254740992": VALUE, "9007199254740993": DEFER,
    "1e22": VALUE, "1e23": DEFER, "1e-22": VALUE, "1e-23": DEFER, "9007199254740992e22": VALUE,
    "0.0000000000000000000001": VALUE,          # q = -22
    "0.00000000000000000000001": DEFER,         # q = -23
    "123.456e24": VALUE,                        # q = 24 - 3 = 21
    "1e400": DEFER, "1e-400": DEFER, "1e99999999999999999999": DEFER,
    ".": REJECT, "e5": REJECT, "1e": REJECT, "1e+": REJECT, "": REJECT, "+": REJECT, "-": REJECT, "1.2.3": REJECT,
    "1e5e5": REJECT, "1-2": REJECT, "--1": REJECT, "1e5.5": REJECT,
    "inf": DEFER, "nan": DEFER, "-inf": DEFER, "Infinity": DEFER, "0x1p-1": DEFER, "0x10": DEFER, " 0.5": DEFER,
    "0.5 ": DEFER, "1_0": DEFER, "1,5": DEFER, "abc": DEFER,
}


def bits(x):
    return struct.pack("<d", float(x))


def hostlib():
    from alphabeta_rs_amd import build as B

    B.build_host()
    L = C.CDLL(str(B.PEDIGREE_LIB))
    ll = C.c_longlong
    p = lambda t: C.POINTER(t)
    site_arrays = [p(ll), p(C.c_int), p(C.c_uint), p(C.c_uint), p(C.c_ubyte), p(C.c_double), p(C.c_ubyte), p(C.c_double)]
    L.abh_parse_sites.argtypes = [C.c_char_p, ll, ll, ll, *site_arrays, p(ll)]
    L.abh_parse_sites.restype = ll
    L.abh_parse_f64_token.argtypes = [C.c_char_p, ll, p(C.c_double)]
    L.abh_parse_f64_token.restype = C.c_int
    L.abh_classify_text.argtypes = [C.c_char_p, ll, ll, ll, p(C.c_ubyte), p(ll), p(C.c_uint), p(C.c_double), p(ll)]
    L.abh_classify_text.restype = ll
    L.abh_parse_sites_device.argtypes = [C.c_char_p, ll, ll, ll, ll, *site_arrays, C.c_char_p, ll]
    L.abh_parse_sites_device.restype = ll
    return L


FIELDS = (("line", np.int64), ("chromosome", np.int32), ("start", np.uint32), ("end", np.uint32), ("strand", np.uint8),
          ("posteriormax", np.float64), ("status", np.uint8), ("meth_lvl", np.float64))


def _site_arrays(L, cap):
    arrays = {k: np.zeros(cap, dtype=t) for k, t in FIELDS}
    return arrays, [a.ctypes.data_as(t) for a, t in zip(arrays.values(), L.abh_parse_sites.argtypes[4:12])]


def host_sites(L, text: bytes, skip_lines=1):
    """parse_sites_host -> (dict of arrays, number of invalid-status warnings)"""
    cap = text.count(b"\n") + 2
    arrays, ptrs = _site_arrays(L, cap)
    nw = C.c_longlong()
    n = L.abh_parse_sites(text, len(text), skip_lines, cap, *ptrs, C.byref(nw))
    assert n >= 0
    return {k: a[:n] for k, a in arrays.items()}, nw.value


def device_sites_merged(L, text: bytes, skip_lines=1, slab_bytes=0):
    """parse_sites_device of the host layer (device records merged with the deferred lines) -> (dict, warnings text)"""
    cap = text.count(b"\n") + 2
    arrays, ptrs = _site_arrays(L, cap)
    warn = C.create_string_buffer(1 << 16)
    n = L.abh_parse_sites_device(text, len(text), skip_lines, slab_bytes, cap, *ptrs, warn, len(warn))
    assert n >= 0, n
    return {k: a[:n] for k, a in arrays.items()}, warn.value.decode(errors="replace")


def classify(L, text: bytes, skip_lines=1):
    """abn_parse_line of every line -> (cls per line from skip_lines on, dict of the sites' arrays with status_flag)"""
    cap = text.count(b"\n") + 2
    cls = np.zeros(cap, dtype=np.uint8)
    line = np.zeros(cap, dtype=np.int64)
    u6 = np.zeros((cap, 6), dtype=np.uint32)
    d2 = np.zeros((cap, 2))
    ns = C.c_longlong()
    p = lambda a, t: a.ctypes.data_as(C.POINTER(t))
    n = L.abh_classify_text(text, len(text), skip_lines, cap, p(cls, C.c_ubyte), p(line, C.c_longlong), p(u6, C.c_uint),
                            p(d2, C.c_double), C.byref(ns))
    assert n >= 0
    k = ns.value
    sites = {"line": line[:k], "chromosome": u6[:k, 0].astype(np.int32), "start": u6[:k, 1].copy(), "end": u6[:k, 2].copy(),
             "strand": u6[:k, 3].astype(np.uint8), "posteriormax": d2[:k, 0].copy(), "status": u6[:k, 4].astype(np.uint8),
             "meth_lvl": d2[:k, 1].copy(), "status_flag": u6[:k, 5].astype(np.uint8)}
    return cls[:n], sites


def token_class(L, tok: bytes):
    v = C.c_double(0.0)
    c = L.abh_parse_f64_token(tok, len(tok), C.byref(v))
    return c, v.value


def assert_sites_equal(got, want, keys=None):
    """record for record, bit for bit (the floats compared as bytes: -0.0 and NaN included)"""
    for k in keys or [k for k, _ in FIELDS]:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.dtype == w.dtype and g.shape == w.shape, (k, g.dtype, w.dtype, g.shape, w.shape)
        assert g.tobytes() == w.tobytes(), (k, [(i, g[i], w[i]) for i in range(len(g))
                                                if g[i:i + 1].tobytes() != w[i:i + 1].tobytes()][:5])


def line_spans(text: bytes):
    """[(offset, length without the line end)] of every line, as BufRead::lines cuts them"""
    spans, b = [], 0
    while b < len(text):
        e = text.find(b"\n", b)
        e = len(text) if e < 0 else e
        n = e - b - (1 if e > b and text[e - 1:e] == b"\r" else 0)
        spans.append((b, n))
        b = e + 1
    return spans


def cg_line(chrom="1", pos="100", strand="+", ctx="CG", cm="3", ct="8", pm="0.9999", st="M", ml="0.5", tri=None):
    f = [chrom, pos, strand, ctx, cm, ct, pm, st, ml] + ([tri] if tri is not None else [])
    return "\t".join(f)


def third_line(chrom="1", first="100", second="102", ctx="CG", what="x", strand="+", cm="3", ct="8", pm="0.9999", st="M",
               ml="0.5"):
    return "\t".join([chrom, first, second, ctx, what, strand, cm, ct, pm, st, ml])


def torture_text():
    """A few hundred lines: every format, every way out of it, every f64 token of TOKENS in both float columns"""
    lines = []
    for ctx in ("CG", "CHH"):
        lines += [cg_line(ctx=ctx), cg_line(ctx=ctx, tri="CGA"), third_line(ctx=ctx)]                 # 9, 10, 11 fields
    lines += ["\t".join(["1", "5", "+", "CG", "1", "2", "0.5", "M"]),                                   # 8 fields
              "\t".join(["1", "5", "7", "CG", "x", "+", "1", "2", "0.5", "M", "0.5", "extra"]),         # 12 fields
              "1 131800 132400", "1 131800 132400 E10", "1 131800 132400 E10 more",                     # 3, 4, 5 by space
              "chr1\t1\t4\t1", "chr1 1\t4 1", "1\t2\t3\t", "1\t\t3\t4", "\t1\t2\t3", "1  2 3",          # mixed, empty fields
              "", "", "\t", " ", "\t\t\t\t\t\t\t\t", "\t\t\t\t\t\t\t\t\t\t"]
    for pos in ("+17", "4294967295", "4294967296", "-1", "", "1x", "+", "00042"):
        lines += [cg_line(pos=pos), third_line(first="1", second=pos), f"1 {pos} 9 s", f"1 9 {pos} s"]
    for chrom in ("chrchr1", "chrM", "C", "255", "256", "chr", "M", "chrC", "chrX", "+5", "CHR1", "chr chr1", "0"):
        lines += [cg_line(chrom=chrom), third_line(chrom=chrom), f"{chrom}\t1\t4\tE1"]
    for st in ("X", "", "U", "I", "M", "Mx", "u", "é"):
        lines += [cg_line(st=st), cg_line(st=st, tri="CGG"), third_line(st=st)]
    for strand in ("*", "-", "+", "", "++"):
        lines += [cg_line(strand=strand), third_line(strand=strand)]
    for cm in ("", "x", "4294967296", "+0"):
        lines += [cg_line(cm=cm), cg_line(ct=cm)]
    for tok in TOKENS:
        lines += [cg_line(pm=tok), cg_line(ml=tok, tri="CGT"), third_line(pm=tok, ml=tok),
                  cg_line(pm=tok, pos="x"), cg_line(ml=tok, st="")]    # rejected for another field whatever the token is
    return (HEADER + "\n".join(lines) + "\n").encode()


def plain_text(n_lines, seed, cg_every=7, eol="\n", final_newline=True):
    """An all-context methylome as the golden files are: about one line in cg_every is CG, four-decimal values (at most 15
    significant digits, no exponent)"""
    rng = np.random.default_rng(seed)
    rows = []
    for i in range(n_lines):
        ctx = "CG" if rng.integers(cg_every) == 0 else ("CHH", "CHG")[int(rng.integers(2))]
        rows.append("\t".join([str(1 + i // 1000000), str(i + 1), "+-"[int(rng.integers(2))], ctx, str(int(rng.integers(30))),
                               str(int(rng.integers(30, 60))), f"{rng.random():.4f}", "UIM"[int(rng.integers(3))],
                               f"{rng.random():.4f}", "CGA"]))
    body = eol.join(rows)
    return (HEADER.replace("\n", eol) + body + (eol if final_newline else "")).encode()
