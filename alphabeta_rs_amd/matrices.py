"""abn_windows, abn_codes and abn_tiles: the device-resident 2-bit packed matrices made from methylome sites."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._ffi import (GeneRule, WindowsParams, _arr, _f64, _Handle, _pair_outputs, _pair_tables, _ptr, _sites_handles)
from .blocks import _block_outputs
from .context import Context
from .sites import Genes, _site_arrays

_ALIGN_CREATE = {"none": "abn_{}_create_parsed", "position": "abn_{}_create_aligned", "union": "abn_{}_create_union"}


def _align_mode(align) -> str:
    """from_parsed's align argument -> "none", "position" or "union" (False / None; True or "position"; "union")"""
    if align is None or align is False or align == "none":
        return "none"
    if align is True or align == "position":
        return "position"
    if align == "union":
        return "union"
    raise ValueError(f"align expects False, True, 'position' or 'union', not {align!r}")


def _windows_params(cutoff, step, size, absolute, counts):
    return WindowsParams(cutoff, step, size, 1 if absolute else 0, *map(int, counts))


class _PackedMatrix(_Handle):
    """What Windows and Codes share: the report of the alignment they were made with, and the packed matrix
    (n_samples, row_stride) they keep on the device.  `_PREFIX` is the C prefix of their entry points."""

    def _aligned(self, entry, n_ms):
        before, each, ms = np.zeros(self.n_samples, dtype=np.int64), C.c_int64(-1), np.zeros(n_ms)
        self._check(self._entry(entry)(self._h, _ptr(before), C.byref(each), _ptr(ms)))
        return before, each.value, ms

    def common(self):
        """(before int64 (n_samples,), n_common, ms (4,)): every sample's sites before the alignment, the sites each keeps
        (-1: not made with align) and the HIP-event ms of the common-site kernels (runs and ends, match, scan and rank,
        gather; zeros without align)"""
        return self._aligned("common", 4)

    def union(self):
        """(before int64 (n_samples,), n_union, ms (8,)): every sample's sites before the alignment, the sites each has
        behind it, placeholders included (-1: not made with align="union") and the HIP-event ms of the union passes (runs
        and ends, owner, scan, base, rank, dest, invert, gather; zeros otherwise)"""
        return self._aligned("union", 8)

    def packed(self) -> np.ndarray:
        """the packed matrix (n_samples, row_stride) uint8, copied to the host"""
        out = np.empty((self.n_samples, self.row_stride), dtype=np.uint8)
        self._check(self._entry("packed")(self._h, _ptr(out)))
        return out

    def packed_device_ptr(self) -> int:
        p = C.c_void_p()
        self._check(self._entry("packed_device_ptr")(self._h, C.byref(p)))
        return p.value or 0


class Windows(_PackedMatrix):
    """abn_windows: the sites of n_samples methylomes placed into metaprofile windows on the device
    (MethylationSite::place_in_windows, src/methylation_site.rs:423-490), device-resident as the 2-bit packed matrix of
    Context.pairwise_divergence_windows_packed.

    site_offset (n_samples + 1,) int64; per site (concatenated over the samples, file order): pos, gene_start, gene_end
    uint32, flags uint8 (bit 0 antisense, bit 1 has a gene), code uint8 (status | 0x80 when filtered), level float64.
    cutoff, step, size, absolute: arguments::Windows; counts = (n_upstream, n_gene, n_downstream) of Windows::new."""

    _DESTROY, _PREFIX = "abn_windows_destroy", "abn_windows"

    def __init__(self, ctx: Context, site_offset, pos, gene_start, gene_end, flags, code, level, *, cutoff, step, size,
                 absolute, counts):
        self.ctx = ctx
        self._L = ctx._L
        off = _arr(site_offset, np.int64)
        self.n_samples = off.shape[0] - 1
        S = int(off[-1]) if off.shape[0] else 0
        u32 = [_arr(a, np.uint32, S) for a in (pos, gene_start, gene_end)]
        u8 = [_arr(a, np.uint8, S) for a in (flags, code)]
        lvl = _f64(level, (S,))
        p = _windows_params(cutoff, step, size, absolute, counts)
        h = C.c_void_p()
        self._check(self._L.abn_windows_create(ctx._h, C.byref(p), self.n_samples, _ptr(off), *map(_ptr, u32),
                                               *map(_ptr, u8), _ptr(lvl), C.byref(h)))
        self._finish(h)

    def _finish(self, h):
        """the handle taken, and what abn_windows_info says of it"""
        self._h = h
        W, stride, ns = C.c_int32(), C.c_int64(), C.c_int64()
        self._check(self._L.abn_windows_info(h, C.byref(W), C.byref(stride), C.byref(ns)))
        self.W, self.row_stride, self.n_sites = W.value, stride.value, ns.value
        return self

    @classmethod
    def from_sites(cls, ctx: Context, genes: Genes, site_offset, chromosome, start, end, strand, code, level, *, cutoff,
                   cutoff_gene_length=False, step, size, absolute, counts):
        """The handle from the sites' own fields (chromosome int32, start, end uint32, strand uint8; code, level as
        above): every site's gene is chosen on the device (Context.choose_genes) and handed to the placement there."""
        self = cls._new(ctx)
        off, u = _site_arrays(site_offset, chromosome, start, end, strand)
        self.n_samples = off.shape[0] - 1
        S = int(off[-1]) if off.shape[0] else 0
        co = _arr(code, np.uint8, S)
        lvl = _f64(level, (S,))
        p = _windows_params(cutoff, step, size, absolute, counts)
        rule = GeneRule(cutoff, 1 if cutoff_gene_length else 0)
        h = C.c_void_p()
        self._check(self._L.abn_windows_create_sites(ctx._h, C.byref(p), genes._h, C.byref(rule), self.n_samples,
                                                     _ptr(off), *map(_ptr, u), _ptr(co), _ptr(lvl), C.byref(h)))
        return self._finish(h)

    @classmethod
    def from_parsed(cls, ctx: Context, genes: Genes, sites_list, *, posterior_max_filter, cutoff,
                    cutoff_gene_length=False, step, size, absolute, counts, align=False):
        """The handle from resident parse results (Context.parse_sites_resident, one Sites per methylome, their deferred
        lines decided and inserted): merged in file order, the genes chosen and the windows placed on the device, no site
        record coming back to the host (abn_windows_create_parsed).  The Sites are not consumed.  align: True or
        "position": only the sites every sample shares (Context.common_sites) are placed (abn_windows_create_aligned);
        "union": every sample gets all the sites any sample holds, filtered placeholders where it lacks one
        (Context.union_sites, abn_windows_create_union).  Either way no window is ragged."""
        self = cls._new(ctx)
        self.n_samples, handles = _sites_handles(sites_list)
        p = _windows_params(cutoff, step, size, absolute, counts)
        rule = GeneRule(cutoff, 1 if cutoff_gene_length else 0)
        h = C.c_void_p()
        create = getattr(self._L, _ALIGN_CREATE[_align_mode(align)].format("windows"))
        self._check(create(ctx._h, C.byref(p), genes._h, C.byref(rule), posterior_max_filter, self.n_samples, handles,
                           C.byref(h)))
        return self._finish(h)

    def merge_ms(self) -> np.ndarray:
        """the HIP-event ms of from_parsed's two merge kernels (fields, insert); zeros for the other forms"""
        return self._ms(self._L.abn_windows_merge_ms, 2)

    def stats(self):
        """(count int64, level_sum, level_sum_kept, kept int64), each (n_samples, W)"""
        shape = (self.n_samples, self.W)
        count, kept = np.zeros(shape, dtype=np.int64), np.zeros(shape, dtype=np.int64)
        ls, lsk = np.zeros(shape), np.zeros(shape)
        self._check(self._L.abn_windows_stats(self._h, _ptr(count), _ptr(ls), _ptr(lsk), _ptr(kept)))
        return count, ls, lsk, kept

    def layout(self):
        """(begin int64, end int64, ragged int32), each (W,): window w = the fields [begin[w], end[w]) of every row"""
        b, e = np.zeros(self.W, dtype=np.int64), np.zeros(self.W, dtype=np.int64)
        r = np.zeros(self.W, dtype=np.int32)
        self._check(self._L.abn_windows_layout(self._h, _ptr(b), _ptr(e), _ptr(r)))
        return b, e, r

    def pairwise(self):
        """(diff, both, dvalue), each (W, pairs): pairwise_divergence of every window, on the resident matrix"""
        diff, both, dval = _pair_outputs(self.n_samples, (self.W,))
        self._check(self._L.abn_windows_pairwise(self._h, _ptr(diff), _ptr(both), _ptr(dval)))
        return diff, both, dval


class Codes(_PackedMatrix):
    """abn_codes: what Pedigree::build reads of n_samples methylomes (src/pedigree.rs:147-172, :245-251), made on the device
    from resident parse results: the 2-bit packed matrix of Context.pairwise_divergence_packed, device-resident, and every
    sample's rc_meth_lvl fold."""

    _DESTROY, _PREFIX = "abn_codes_destroy", "abn_codes"

    @classmethod
    def from_parsed(cls, ctx: Context, sites_list, *, posterior_max_filter, align=False):
        """From resident parse results (Context.parse_sites_resident with skip_lines 0 for the pedigree build, one Sites
        per methylome, their deferred lines decided and inserted): merged in file order, packed and folded on the device,
        no site record coming back to the host (abn_codes_create_parsed).  The Sites are not consumed.  align: only the
        sites every sample shares (Context.common_sites) are packed and folded (abn_codes_create_aligned): the samples have
        the same length then, and stats() describes the aligned sites.  align="union": every sample gets all the sites any
        sample holds, filtered placeholders where it lacks one (abn_codes_create_union): count is n_union, kept and the
        level sums are the unaligned handle's, and a pair is compared on the sites both hold."""
        self = cls._new(ctx)
        n, handles = _sites_handles(sites_list)
        h = C.c_void_p()
        create = getattr(self._L, _ALIGN_CREATE[_align_mode(align)].format("codes"))
        self._check(create(ctx._h, posterior_max_filter, n, handles, C.byref(h)))
        self._h = h
        i = self.info()
        self.n_samples, self.n_sites, self.row_stride, self.same_len = i["n_samples"], i["n_sites"], i["row_stride"], i["same_len"]
        return self

    def info(self):
        """{n_samples, n_sites (of the longest sample), row_stride (bytes), same_len (bool)}"""
        n, same, ns, stride = C.c_int32(), C.c_int32(), C.c_int64(), C.c_int64()
        self._check(self._L.abn_codes_info(self._h, C.byref(n), C.byref(ns), C.byref(stride), C.byref(same)))
        return {"n_samples": n.value, "n_sites": ns.value, "row_stride": stride.value, "same_len": bool(same.value)}

    def stats(self):
        """(count int64, level_sum_kept, kept int64), each (n_samples,): a sample's sites, and the sum and number of the
        levels whose posterior passes the filter (rc_meth_lvl = level_sum_kept / kept)"""
        count, kept = np.zeros(self.n_samples, dtype=np.int64), np.zeros(self.n_samples, dtype=np.int64)
        lsk = np.zeros(self.n_samples)
        self._check(self._L.abn_codes_stats(self._h, _ptr(count), _ptr(lsk), _ptr(kept)))
        return count, lsk, kept

    def pairwise(self):
        """(diff, both, dvalue), each (pairs,): pairwise_divergence_packed on the resident matrix; refused (AbnError) when
        the samples differ in length"""
        diff, both, dval = _pair_outputs(self.n_samples)
        self._check(self._L.abn_codes_pairwise(self._h, _ptr(diff), _ptr(both), _ptr(dval)))
        return diff, both, dval

    def transitions(self):
        """uint64 (pairs, 3, 3): Context.pairwise_transitions_packed on the resident matrix (under a union alignment the
        placeholder sites count in no entry); refused (AbnError) when the samples differ in length"""
        table = _pair_tables(self.n_samples)
        self._check(self._L.abn_codes_transitions(self._h, _ptr(table)))
        return table

    def kernel_ms(self) -> np.ndarray:
        """the HIP-event ms of from_parsed's kernels: merge of the records, merge of the inserted lines, pack, fold"""
        return self._ms(self._L.abn_codes_kernel_ms, 4)


class Tiles(_Handle):
    """abn_tiles: Pedigree::build (src/pedigree.rs:147-172, :210-261) once per genomic tile — a fixed bin or a listed region
    (the region rows of src/cli/metaprofile.rs:50-72) — over resident parse results: the aligned code matrix, its columns'
    keys and every sample's merged bytes and levels stay on the device; a tile is a contiguous column range.  set_pools makes
    a set of intervals one tile: its columns gathered into a pooled matrix (one pedigree per annotation class)."""

    _DESTROY = "abn_tiles_destroy"
    ALIGN = {"none": 0, "position": 1, "union": 2}

    @classmethod
    def from_parsed(cls, ctx: Context, sites_list, *, posterior_max_filter, align=False):
        """From resident parse results, as Codes.from_parsed (abn_tiles_create).  align False / "none": the reference's
        assumption that site k is the same site in every sample — the keys are sample 0's and every sample must have its
        number of sites; True / "position": the sites every sample shares; "union": every site any sample holds, filtered
        and uncounted placeholders where a sample lacks one."""
        self = cls._new(ctx)
        n, handles = _sites_handles(sites_list)
        h = C.c_void_p()
        self._check(self._L.abn_tiles_create(ctx._h, posterior_max_filter, cls.ALIGN[_align_mode(align)], n, handles,
                                             C.byref(h)))
        self._h = h
        i = self.info()
        self.n_samples, self.n_columns, self.row_stride, self.n_runs = i["n_samples"], i["n_columns"], i["row_stride"], i["n_runs"]
        return self

    def info(self):
        """{n_samples, n_columns, row_stride (bytes), n_runs, n_tiles (-1 before set_intervals / set_fixed)}"""
        n, runs, cols, stride, tiles = C.c_int32(), C.c_int32(), C.c_int64(), C.c_int64(), C.c_int64()
        self._check(self._L.abn_tiles_info(self._h, C.byref(n), C.byref(cols), C.byref(stride), C.byref(runs), C.byref(tiles)))
        return {"n_samples": n.value, "n_columns": cols.value, "row_stride": stride.value, "n_runs": runs.value,
                "n_tiles": tiles.value}

    def runs(self):
        """(chromosome int32, first int64, count int64, last_start uint32), each (n_runs,): the chromosome runs of the
        columns in run order, and the start of every run's last column"""
        chrom, last = np.zeros(self.n_runs, dtype=np.int32), np.zeros(self.n_runs, dtype=np.uint32)
        first, count = np.zeros(self.n_runs, dtype=np.int64), np.zeros(self.n_runs, dtype=np.int64)
        self._check(self._L.abn_tiles_runs(self._h, _ptr(chrom), _ptr(first), _ptr(count), _ptr(last)))
        return chrom, first, count, last

    def set_intervals(self, chromosome, start, end):
        """the tiles (chromosome 0..257, start, end), half-open on a site's start, bounds in [0, 2^32]: the search and the
        per-(sample, tile) folds run on the device; a new list replaces the old"""
        chrom = _arr(chromosome, np.int32, -1)
        lo, hi = (_arr(a, np.int64, -1) for a in (start, end))
        if not chrom.shape == lo.shape == hi.shape:
            raise ValueError("chromosome, start and end differ in length")
        self._check(self._L.abn_tiles_set_intervals(self._h, chrom.shape[0], _ptr(chrom), _ptr(lo), _ptr(hi)))

    def set_fixed(self, size, step=0):
        """fixed tiles: for every run in run order [k step, k step + size), k = 0 .. ceil((last_start + 1) / step) - 1
        (step 0: size)"""
        self._check(self._L.abn_tiles_set_fixed(self._h, int(size), int(step)))

    def set_pools(self, chromosome, start, end, pool, n_pools):
        """pools of intervals (abn_tiles_set_pools): interval k belongs to pool[k] in [0, n_pools); a pool's columns are
        those inside at least one of its intervals, each once, in column order, gathered into a pooled matrix on the
        device.  Afterwards the tiles are the pools: layout() is in pooled column space, stats() and pairwise() per pool"""
        chrom, ids = (_arr(a, np.int32, -1) for a in (chromosome, pool))
        lo, hi = (_arr(a, np.int64, -1) for a in (start, end))
        if not chrom.shape == lo.shape == hi.shape == ids.shape:
            raise ValueError("chromosome, start, end and pool differ in length")
        self._check(self._L.abn_tiles_set_pools(self._h, chrom.shape[0], _ptr(chrom), _ptr(lo), _ptr(hi), _ptr(ids),
                                                int(n_pools)))

    def pool_segments(self):
        """(pool int32, chromosome int32, start int64, end int64, col_begin int64, col_end int64), each (n_segments,): the
        pools' merged intervals in segment order and their columns of the handle's own matrix"""
        n = C.c_int64()
        self._check(self._L.abn_tiles_pool_segments(self._h, C.byref(n), None, None, None, None, None, None))
        pool, chrom = np.zeros(n.value, dtype=np.int32), np.zeros(n.value, dtype=np.int32)
        lo, hi, cb, ce = (np.zeros(n.value, dtype=np.int64) for _ in range(4))
        self._check(self._L.abn_tiles_pool_segments(self._h, None, *map(_ptr, (pool, chrom, lo, hi, cb, ce))))
        return pool, chrom, lo, hi, cb, ce

    def pool_columns(self):
        """int64 (pooled columns,): every pooled column's source column of the handle's own matrix"""
        self._check(self._L.abn_tiles_pool_segments(self._h, None, None, None, None, None, None, None))   # pools, or refused
        end = self.layout()[1]
        src = np.zeros(int(end[-1]) if len(end) else 0, dtype=np.int64)
        self._check(self._L.abn_tiles_pool_columns(self._h, _ptr(src)))
        return src

    def pool_kernel_ms(self) -> np.ndarray:
        """the HIP-event ms of the last set_pools: offsets, map, gather, pack (search and fold: kernel_ms)"""
        return self._ms(self._L.abn_tiles_pool_kernel_ms, 4)

    def _n_tiles(self):
        return max(self.info()["n_tiles"], 0)

    def intervals(self):
        """(chromosome int32, start int64, end int64), each (n_tiles,)"""
        T = self._n_tiles()
        chrom, lo, hi = np.zeros(T, dtype=np.int32), np.zeros(T, dtype=np.int64), np.zeros(T, dtype=np.int64)
        self._check(self._L.abn_tiles_intervals(self._h, _ptr(chrom), _ptr(lo), _ptr(hi)))
        return chrom, lo, hi

    def layout(self):
        """(begin int64, end int64), each (n_tiles,): every tile's columns [begin, end)"""
        T = self._n_tiles()
        begin, end = np.zeros(T, dtype=np.int64), np.zeros(T, dtype=np.int64)
        self._check(self._L.abn_tiles_layout(self._h, _ptr(begin), _ptr(end)))
        return begin, end

    def stats(self):
        """(count int64 (n_tiles,), level_sum_kept (n_samples, n_tiles), kept int64 (n_samples, n_tiles)): a tile's columns,
        and per sample the sum and number of the tile's levels whose posterior passes the filter"""
        T = self._n_tiles()
        count, kept = np.zeros(T, dtype=np.int64), np.zeros((self.n_samples, T), dtype=np.int64)
        lsk = np.zeros((self.n_samples, T))
        self._check(self._L.abn_tiles_stats(self._h, _ptr(count), _ptr(lsk), _ptr(kept)))
        return count, lsk, kept

    def pairwise(self):
        """(diff, both, dvalue), each (n_tiles, pairs): pairwise_divergence_windows_packed on the resident matrix over the
        tiles' columns"""
        diff, both, dval = _pair_outputs(self.n_samples, (self._n_tiles(),))
        self._check(self._L.abn_tiles_pairwise(self._h, _ptr(diff), _ptr(both), _ptr(dval)))
        return diff, both, dval

    def transitions(self):
        """uint64 (n_tiles, pairs, 3, 3): Context.pairwise_transitions_windows_packed on the resident matrix over the
        tiles' columns (with pools set: the pooled matrix, one table per pool)"""
        table = _pair_tables(self.n_samples, (self._n_tiles(),))
        self._check(self._L.abn_tiles_transitions(self._h, _ptr(table)))
        return table

    def kernel_ms(self) -> np.ndarray:
        """the HIP-event ms of the last set_intervals / set_fixed: search, fold"""
        return self._ms(self._L.abn_tiles_kernel_ms, 2)

    def block_groups(self):
        """(group_begin, group_end) of block_bootstrap's groups in block space (abn_tiles_block_groups): with pools set every
        pool's segments (in pool_segments order), else the one group of all tiles"""
        G = C.c_int64()
        self._check(self._L.abn_tiles_block_groups(self._h, C.byref(G), None, None, None))
        gb, ge = np.zeros(G.value, dtype=np.int64), np.zeros(G.value, dtype=np.int64)
        self._check(self._L.abn_tiles_block_groups(self._h, None, None, _ptr(gb), _ptr(ge)))
        return gb, ge

    def block_bootstrap(self, seed: int, n_replicates: int):
        """The block bootstrap of the handle's tiles (abn_tiles_block_bootstrap): the blocks — a pooled handle's merged
        segments, one group per pool, or the fixed, non-overlapping tiles in one group — drawn with replacement
        n_replicates times per group; refused on tiles that may overlap.  Returns {both, diff, dvalue: (G, n_replicates +
        1, pairs); level, kept: (G, n_replicates + 1, n_samples)}; the last row of a group is the observed data."""
        n = self.n_samples
        out = _block_outputs(len(self.block_groups()[0]), max(int(n_replicates) + 1, 0), n * (n - 1) // 2, n)
        self._check(self._L.abn_tiles_block_bootstrap(self._h, int(seed), int(n_replicates), *map(_ptr, out.values())))
        return out

    def block_ms(self) -> np.ndarray:
        """the HIP-event ms of the last block_bootstrap: counts, digits, product, finish, levels"""
        return self._ms(self._L.abn_tiles_block_ms, 5)
