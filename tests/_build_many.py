"""Shared by tests/test_pedigree_build_many.py (CPU tier) and tests/test_pairwise_windows.py (GPU): window directories
as src/setup.rs writes them, every window with methylome files of its own, and the two shims of
alphabeta_rs_amd/host/host_capi.cpp (abh_pedigree_build: Pedigree::build's host loop; abh_pedigree_build_many)."""
import ctypes as C

import numpy as np

CAP, ERRCAP = 64, 512
SAMPLES = ["G0.txt", "G1_2.txt", "G4_2.txt", "G4_8.txt"]          # the "Y" rows of data/nodelist.txt


def hostlib():
    from alphabeta_rs_amd import build as B

    B.build_host()
    L = C.CDLL(str(B.PEDIGREE_LIB))
    L.abh_pedigree_build.argtypes = [C.c_char_p, C.c_char_p, C.c_double, C.POINTER(C.c_double), C.c_int,
                                     C.POINTER(C.c_double), C.c_char_p, C.c_int]
    L.abh_pedigree_build_many.argtypes = [C.POINTER(C.c_char_p), C.POINTER(C.c_char_p), C.c_int, C.c_double, C.c_int,
                                          C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_int),
                                          C.c_char_p, C.c_int]
    return L


def write_windows(tmp_path, golden_dir):
    """Seven window directories -> [(nodelist, edgelist)].  Window k's methylomes are the CG rows [30 k, 30 k + 120 + 30 k)
    of the bundled ones' 500 (other site counts, other content); window 2 has no nodelist, window 3 samples three nodes only
    (another topology), window 5's last sample is 40 rows shorter (the "Lengths do not match" path)."""
    src = {f: (golden_dir / "data" / "methylome" / f).read_text().splitlines(keepends=True) for f in
           ["G0.txt", "G1_2.txt", "G1_8.txt", "G2_2.txt", "G2_8.txt", "G4_2.txt", "G4_8.txt"]
           if (golden_dir / "data" / "methylome" / f).exists()}
    nodes = (golden_dir / "data" / "nodelist.txt").read_text()
    lists = []
    for k in range(7):
        d = tmp_path / "gene" / str(k)
        (d / "methylome").mkdir(parents=True)
        lists.append((str(d / "nodelist.txt"), str(d / "edgelist.txt")))
        if k == 2:
            continue
        (d / "edgelist.txt").write_text((golden_dir / "data" / "edgelist.txt").read_text())
        text = nodes
        for f, lines in src.items():
            cg = [ln for ln in lines[1:] if ln.split("\t")[3] == "CG"]
            hi = 30 * k + 120 + 30 * k - (40 if (k == 5 and f == "G4_8.txt") else 0)
            (d / "methylome" / f).write_text("".join(lines[:1] + cg[30 * k: hi]))
            text = text.replace("./data/methylome/" + f, str(d / "methylome" / f))
        if k == 3:
            text = text.replace("G4_8.txt,4_8,4,Y", "G4_8.txt,4_8,4,N")
        (d / "nodelist.txt").write_text(text)
    return lists


def build_each(L, lists, flt=0.99):
    """Pedigree::build (host loop) per entry -> [(rows or -1, rows array, p0uu, error text)]"""
    out = []
    for nl, el in lists:
        rows, p0, err = np.zeros((CAP, 4)), C.c_double(), C.create_string_buffer(ERRCAP)
        n = L.abh_pedigree_build(nl.encode(), el.encode(), flt, rows.ctypes.data_as(C.POINTER(C.c_double)), CAP,
                                 C.byref(p0), err, ERRCAP)
        out.append((n, rows[:max(n, 0)].copy(), p0.value if n >= 0 else None, err.value))
    return out


def build_many(L, lists, gpu, flt=0.99):
    W = len(lists)
    nls = (C.c_char_p * W)(*[a.encode() for a, _ in lists])
    els = (C.c_char_p * W)(*[b.encode() for _, b in lists])
    rows, p0, nrows = np.zeros((W, CAP, 4)), np.zeros(W), (C.c_int * W)()
    errs = C.create_string_buffer(W * ERRCAP)
    rc = L.abh_pedigree_build_many(nls, els, W, flt, 1 if gpu else 0, rows.ctypes.data_as(C.POINTER(C.c_double)), CAP,
                                   p0.ctypes.data_as(C.POINTER(C.c_double)), nrows, errs, ERRCAP)
    assert rc == 0
    raw = errs.raw
    return [(nrows[w], rows[w, :max(nrows[w], 0)].copy(), p0[w] if nrows[w] >= 0 else None,
             raw[w * ERRCAP:(w + 1) * ERRCAP].split(b"\0", 1)[0]) for w in range(W)]
