"""What the context tests share (tests/test_sites_split_cpu.py, tests/test_sites_split_gpu.py): the masked host shims of
host_capi.cpp, the relabel oracle — a text rewritten so that the CG-only parser of the parent behaviour reads one other
context — and the texts both files run on."""
import ctypes as C
from functools import lru_cache

import numpy as np

import _parse_model as P

CONTEXTS = ("CG", "CHG", "CHH")
MASKS = tuple(range(1, 8))
GOLDEN_COUNTS = {1: 500, 2: 400, 4: 1900, 7: 2800}      # the sites of every golden methylome, skip_lines = 1
OTHER_CONTEXTS = ("CH", "CGG", "cg", "")                 # no context at all: such a line is no site under any mask


def hostlib():
    L = P.hostlib()
    ll, p = C.c_longlong, C.POINTER
    site_arrays = L.abh_parse_sites.argtypes[4:12]
    L.abh_parse_sites_ctx.argtypes = [C.c_char_p, ll, ll, C.c_uint, ll, *site_arrays, p(C.c_ubyte), p(ll)]
    L.abh_parse_sites_ctx.restype = ll
    L.abh_classify_text_ctx.argtypes = [C.c_char_p, ll, ll, C.c_uint, ll, p(C.c_ubyte), p(ll), p(C.c_uint), p(C.c_double),
                                        p(C.c_ubyte), p(ll)]
    L.abh_classify_text_ctx.restype = ll
    u32p, dp = p(C.c_uint), p(C.c_double)
    L.abh_sites_split_serial.argtypes = [C.c_int, C.c_uint, p(ll), u32p, u32p, u32p, u32p, dp, dp, u32p, u32p, u32p, u32p, u32p, dp, dp]
    L.abh_sites_split_serial.restype = ll
    return L


def host_sites(L, text: bytes, mask: int, skip_lines=1):
    """parse_sites_host under a context mask -> the dict of P.host_sites with `context` beside it"""
    cap = text.count(b"\n") + 2
    arrays, ptrs = P._site_arrays(L, cap)
    ctx = np.zeros(cap, dtype=np.uint8)
    nw = C.c_longlong()
    n = L.abh_parse_sites_ctx(text, len(text), skip_lines, mask, cap, *ptrs, ctx.ctypes.data_as(C.POINTER(C.c_ubyte)),
                              C.byref(nw))
    assert n >= 0
    out = {k: a[:n] for k, a in arrays.items()}
    out["context"] = ctx[:n]
    return out


def classify(L, text: bytes, mask: int, skip_lines=1):
    """abn_parse_line under a context mask -> (cls per line from skip_lines on, the sites' arrays with `context`)"""
    cap = text.count(b"\n") + 2
    cls, line = np.zeros(cap, dtype=np.uint8), np.zeros(cap, dtype=np.int64)
    u6, d2, ctx = np.zeros((cap, 6), dtype=np.uint32), np.zeros((cap, 2)), np.zeros(cap, dtype=np.uint8)
    ns = C.c_longlong()
    p = lambda a, t: a.ctypes.data_as(C.POINTER(t))
    n = L.abh_classify_text_ctx(text, len(text), skip_lines, mask, cap, p(cls, C.c_ubyte), p(line, C.c_longlong),
                                p(u6, C.c_uint), p(d2, C.c_double), p(ctx, C.c_ubyte), C.byref(ns))
    assert n >= 0
    k = ns.value
    sites = {"line": line[:k], "chromosome": u6[:k, 0].astype(np.int32), "start": u6[:k, 1].copy(), "end": u6[:k, 2].copy(),
             "strand": u6[:k, 3].astype(np.uint8), "posteriormax": d2[:k, 0].copy(), "status": u6[:k, 4].astype(np.uint8),
             "meth_lvl": d2[:k, 1].copy(), "status_flag": u6[:k, 5].astype(np.uint8), "context": ctx[:k]}
    return cls[:n], sites


def relabel(text: bytes, c: int) -> bytes:
    """Field 3 of every line of at least 9 tab-separated fields rewritten: context c becomes CG and, when c is not CG, CG
    becomes XX.  The CG-only parser reads on the result what the parser of context c reads on the text."""
    want = CONTEXTS[c].encode()
    lines = text.split(b"\n")
    for i, line in enumerate(lines):
        f = line.split(b"\t")
        if len(f) < 9:
            continue
        if f[3] == want:
            f[3] = b"CG"
        elif f[3] == b"CG":
            f[3] = b"XX"
        lines[i] = b"\t".join(f)
    return b"\n".join(lines)


def line_contexts(text: bytes):
    """field 3 of every line with 9 to 11 tab-separated fields (None for any other line), a line per '\\n'"""
    out = []
    for line in text.split(b"\n"):
        f = line.split(b"\t")
        out.append(f[3].decode(errors="replace") if 9 <= len(f) <= 11 else None)
    return out


@lru_cache(maxsize=None)
def torture_text() -> bytes:
    """every line of P.torture_text, those with a context field once per context and per OTHER_CONTEXTS"""
    head, *body = P.torture_text().decode().split("\n")
    assert body[-1] == ""
    lines = []
    for line in body[:-1]:
        f = line.split("\t")
        if len(f) >= 9:
            for ctx in CONTEXTS + OTHER_CONTEXTS:
                lines.append("\t".join(f[:3] + [ctx] + f[4:]))
        else:
            lines.append(line)
    return ("\n".join([head] + lines) + "\n").encode()


def rows_only_text(n=300) -> bytes:
    """4-field chromatin-state rows alone: no line has a context, every mask accepts them all"""
    return (P.HEADER + "".join(f"chr{1 + i % 5}\t{10 * i}\t{10 * i + 7}\tE{i % 9}\n" for i in range(n))).encode()


@lru_cache(maxsize=None)
def texts():
    """(name, text) of every text the issue names"""
    return tuple([("methylome " + p.name, p.read_bytes()) for p in P.GOLDEN_METHYLOMES] + [("torture", torture_text())] +
                 [(f"plain {n}", P.plain_text(n, seed=n, cg_every=3)) for n in (255, 256, 257, 1025)])


def decide(L, text: bytes, deferred, mask: int):
    """masked parse_site_full on every deferred line -> the arrays Sites.insert takes, `context` last"""
    keys = ("chromosome", "start", "end", "strand", "posteriormax", "status", "meth_lvl", "context")
    rows = []
    for line, off, n in zip(*(deferred[k].tolist() for k in ("line", "offset", "length"))):
        s = host_sites(L, text[off:off + n], mask, skip_lines=0)
        assert len(s["line"]) <= 1
        if len(s["line"]):
            rows.append((line, *(s[k][0] for k in keys)))
    cols = list(zip(*rows)) if rows else [[]] * 9
    return [np.array(c, dtype=t) for c, t in zip(cols, (np.int64, np.int32, np.uint32, np.uint32, np.uint8, np.float64,
                                                        np.uint8, np.float64, np.uint8))]
