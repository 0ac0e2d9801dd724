"""abn_sites and abn_genes: resident parse results of a methylome text and a resident gene annotation."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._ffi import _Handle, _arr, _ok, _ptr, _sort_info, load_host_library

CONTEXTS = ("CG", "CHG", "CHH")  # a site's context code indexes it; code 3: a row without a context


def _context_mask(contexts) -> int:
    """("CG", "CHH") or "CG,CHH" or the mask itself -> abn_sites_params.contexts (1 CG, 2 CHG, 4 CHH)"""
    if isinstance(contexts, (int, np.integer)):
        return int(contexts)
    names = contexts.split(",") if isinstance(contexts, str) else list(contexts)
    if not names or len(set(names)) != len(names) or any(n not in CONTEXTS for n in names):
        raise ValueError(f"contexts expects distinct names of {CONTEXTS}, not {contexts!r}")
    return sum(1 << CONTEXTS.index(n) for n in names)


def _site_arrays(site_offset, chromosome, start, end, strand):
    off = _arr(site_offset, np.int64)
    S = int(off[-1]) if off.shape[0] else 0
    return off, [_arr(a, t, S) for a, t in
                 ((chromosome, np.int32), (start, np.uint32), (end, np.uint32), (strand, np.uint8))]


class Sites(_Handle):
    """abn_sites: the parse results of one methylome text (Context.parse_sites_resident: the records resident on the
    device until close())."""

    _DESTROY = "abn_sites_destroy"
    KINDS = {"line": np.int64, "chromosome": np.int32, "start": np.uint32, "end": np.uint32, "strand": np.uint8,
             "posteriormax": np.float64, "status": np.uint8, "status_flag": np.uint8, "meth_lvl": np.float64}

    def __init__(self, ctx: "Context", handle):
        self.ctx, self._L, self._h = ctx, ctx._L, handle

    def info(self):
        """{n_sites (the device's records plus the inserted ones), n_deferred, n_lines, kernel_ms}"""
        n, nd, nl, ms = C.c_int64(), C.c_int64(), C.c_int64(), C.c_double()
        self._check(self._L.abn_sites_info(self._h, C.byref(n), C.byref(nd), C.byref(nl), C.byref(ms)))
        return {"n_sites": n.value, "n_deferred": nd.value, "n_lines": nl.value, "kernel_ms": ms.value}

    def deferred(self):
        """{line, offset, length} of the lines left to the host's parser, in file order"""
        out = {k: np.zeros(self.info()["n_deferred"], dtype=np.int64) for k in ("line", "offset", "length")}
        self._check(self._L.abn_sites_deferred(self._h, *map(_ptr, out.values())))
        return out

    def _listed(self, entry):
        """the int64 list of an entry point (handle, n*, list*), asked for its length first"""
        n = C.c_int64()
        self._check(entry(self._h, C.byref(n), None))
        out = np.zeros(n.value, dtype=np.int64)
        self._check(entry(self._h, None, _ptr(out)))
        return out

    def flagged(self) -> np.ndarray:
        """the file lines of the records whose status byte was none of M, I, U, ascending"""
        return self._listed(self._L.abn_sites_flagged)

    def insert(self, line, chromosome, start, end, strand, posteriormax, status, meth_lvl, context=None):
        """the deferred lines the host's parser accepted, ascending by line; once per handle (abn_sites_insert).  context:
        every record's code (abn_sites_insert_ctx); None is code 0 for all, which a handle of other contexts than CG
        refuses."""
        arrays = [_arr(a, t, -1) for a, t in
                  zip((line, chromosome, start, end, strand, posteriormax, status, meth_lvl),
                      (np.int64, np.int32, np.uint32, np.uint32, np.uint8, np.float64, np.uint8, np.float64))]
        call = self._L.abn_sites_insert
        if context is not None:
            arrays.append(_arr(context, np.uint8, -1))
            call = self._L.abn_sites_insert_ctx
        if len({a.shape[0] for a in arrays}) != 1:
            raise ValueError("the arrays are of one length")
        self._check(call(self._h, arrays[0].shape[0], *map(_ptr, arrays)))

    def mask(self) -> int:
        """the contexts the handle was parsed under (1 CG, 2 CHG, 4 CHH)"""
        m = C.c_int32()
        self._check(self._L.abn_sites_context(self._h, C.byref(m), None))
        return m.value

    def contexts(self) -> np.ndarray:
        """every site's context code in the order of fetch(): 0 CG, 1 CHG, 2 CHH, 3 a row without one"""
        out = np.zeros(self.info()["n_sites"], dtype=np.uint8)
        self._check(self._L.abn_sites_context(self._h, None, _ptr(out)))
        return out

    def split(self) -> "dict[str, Sites]":
        """One resident handle per context of the handle's mask, partitioned on the device (abn_sites_split): each holds
        what parse_sites_resident of the same text with that context alone, its deferred lines inserted, holds, and goes
        into Windows.from_parsed, Codes.from_parsed and Tiles as it is.  This handle stays usable."""
        out = (C.c_void_p * 3)()
        self._check(self._L.abn_sites_split(self._h, out))
        return {name: Sites(self.ctx, C.c_void_p(h)) for name, h in zip(CONTEXTS, out) if h}

    def split_ms(self):
        """(count kernel ms, scatter kernel ms) of the last split() of this handle, or of the split that made it"""
        ms = self._ms(self._L.abn_sites_split_ms, 2)
        return float(ms[0]), float(ms[1])

    def sort(self) -> "Sites":
        """A new resident handle with this handle's sites — device records and inserted ones — in canonical order:
        ascending chromosome key, start, end, strand, equal keys in file order (abn_sites_sort: a stable radix sort on the
        device).  Its lines are 0 .. n_sites - 1; it goes into Windows.from_parsed, Codes.from_parsed, Tiles and split() as
        it is.  This handle stays usable."""
        out = C.c_void_p()
        self._check(self._L.abn_sites_sort(self._h, C.byref(out)))
        return Sites(self.ctx, out)

    def sort_order(self) -> np.ndarray:
        """of a handle sort() made: the index, in the parent's fetch(), of every site (abn_sites_sort_order)"""
        return self._listed(self._L.abn_sites_sort_order)

    def sort_info(self):
        """of a handle sort() made: {sites, descents, equal (neighbours of the input), passes (radix passes run), ms: the
        HIP-event ms of flatten, check, passes, gather}"""
        info, ms = np.zeros(4, dtype=np.int64), np.zeros(4)
        self._check(self._L.abn_sites_sort_info(self._h, _ptr(info), _ptr(ms)))
        return {**_sort_info(info), "ms": ms}

    def fetch(self):
        """the sites in file order as a dict of arrays (Context.parse_sites' fields); a resident handle downloads them and
        merges the inserted records in by line"""
        sites = {k: np.zeros(self.info()["n_sites"], dtype=t) for k, t in self.KINDS.items()}
        self._check(self._L.abn_sites_fetch(self._h, *map(_ptr, sites.values())))
        return sites


class Genes(_Handle):
    """abn_genes: a gene annotation resident on the device.  lists = [(chromosome, kind, start, end, strand), ..]: the
    genes of one chromosome (0..255, 256 = M, 257 = C) and kind (0 sense, 1 antisense, 2 combined: GenesByStrand,
    src/genes.rs:127-163) as arrays, each list stably sorted by start as src/extract.rs:61-66 leaves it."""

    _DESTROY = "abn_genes_destroy"

    def __init__(self, ctx: "Context", lists):
        self.ctx = ctx
        self._L = ctx._L
        lists = list(lists)
        chrom = np.array([l[0] for l in lists], dtype=np.int32)
        kind = np.array([l[1] for l in lists], dtype=np.int32)
        off = np.zeros(len(lists) + 1, dtype=np.int64)
        off[1:] = np.cumsum([len(l[2]) for l in lists])
        cat = lambda k, t: np.ascontiguousarray(np.concatenate([np.asarray(l[k], dtype=t) for l in lists])
                                                if lists else np.zeros(0, dtype=t))
        start, end, strand = cat(2, np.uint32), cat(3, np.uint32), cat(4, np.uint8)
        h = C.c_void_p()
        self._check(self._L.abn_genes_create(ctx._h, len(lists), _ptr(chrom), _ptr(kind), _ptr(off), _ptr(start),
                                             _ptr(end), _ptr(strand), C.byref(h)))
        self._h = h
        self.n_genes = int(off[-1])


def sort_sites_host(chromosome, start, end, strand):
    """Context.sort_sites in its serial host form (abn_sites_sort_keys_host): no device needed; the same refusals, and
    info's passes = the radix passes the device would run"""
    n = np.asarray(chromosome).reshape(-1).shape[0]
    _, u = _site_arrays([0, n], chromosome, start, end, strand)
    order, info = np.zeros(n, dtype=np.int64), np.zeros(4, dtype=np.int64)
    H = load_host_library()
    H.abn_sites_sort_keys_host.argtypes = [C.c_longlong] + [C.c_void_p] * 6
    _ok(H.abn_sites_sort_keys_host(n, *(a.ctypes.data for a in (*u, order, info))),
        "a chromosome outside 0..257 or a strand above 2")
    return order, _sort_info(info)
