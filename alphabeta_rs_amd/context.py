"""abn_ctx — `Context`, one HIP device and stream with every entry point that takes it — and the module-level functions
that need no handle (host arithmetic of the library)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._ffi import (FIT_INFO_DTYPE, AbnError, GeneRule, Options, SitesParams, _arr, _dev, _f64, _ok, _opt, _pair_outputs,
                   _pair_tables, _ptr, _sort_info, _window_ranges, load_library)
from .blocks import _block_arguments, _block_counts_array, _block_groups, _block_outputs, _block_pointers
from .sites import Sites, _context_mask, _site_arrays


def default_options(**kw) -> Options:
    o = Options()
    load_library().abn_default_options(C.byref(o))
    for k, v in kw.items():
        if not hasattr(o, k):
            raise TypeError(f"unknown option {k}")
        setattr(o, k, v)
    return o


def device_count() -> int:
    n = C.c_int(0)
    load_library().abn_device_count(C.byref(n))
    return n.value


def gen_start_simplices(seed: int, window: int, n_starts: int, max_divergence: float) -> np.ndarray:
    out = np.empty((n_starts, 5, 4))
    _ok(load_library().abn_gen_start_simplices(seed, window, n_starts, max_divergence, _ptr(out)))
    return out


def gen_boot_simplices(seed: int, window: int, b0: int, nb: int, params) -> np.ndarray:
    p = _f64(params, (4,))
    out = np.empty((nb, 5, 4))
    _ok(load_library().abn_gen_boot_simplices(seed, window, b0, nb, _ptr(p), _ptr(out)))
    return out


def packed_row_stride(n_sites: int) -> int:
    """Bytes per row of 2-bit packed codes for n_sites sites: ceil(n_sites / 256) * 64 (host arithmetic)."""
    return int(load_library().abn_packed_row_stride(int(n_sites)))


def pack_codes(codes, row_stride: int | None = None) -> np.ndarray:
    """(n_samples, n_sites) u8 codes (status | 0x80 if filtered) -> (n_samples, row_stride) u8 rows of 2-bit fields, the
    input of Context.pairwise_divergence_packed (format: include/abneutral.h).  row_stride: a multiple of 64, default
    packed_row_stride(n_sites).  Host arithmetic; a byte that is no code raises AbnError."""
    codes = _arr(codes, np.uint8)
    n, L = codes.shape
    stride = packed_row_stride(L) if row_stride is None else int(row_stride)
    packed = np.empty((n, max(stride, 0)), dtype=np.uint8)
    _ok(load_library().abn_pack_codes(_ptr(codes), n, L, L, _ptr(packed), stride),
        "pack_codes: a byte that is not 0, 1, 2 or 0x80 | status, or a bad row stride")
    return packed


def unpack_codes(packed, n_sites: int) -> np.ndarray:
    """(n_samples, row_stride) packed rows -> (n_samples, n_sites) u8 codes; filtered sites come back as 0x80."""
    packed = _arr(packed, np.uint8)
    n, stride = packed.shape
    codes = np.empty((n, int(n_sites)), dtype=np.uint8)
    _ok(load_library().abn_unpack_codes(_ptr(packed), n, int(n_sites), stride, _ptr(codes), int(n_sites)),
        "unpack_codes: bad row stride")
    return codes


def analyze(raw) -> np.ndarray:
    """src/analysis.rs:50-98 -> (4, 8): mean, sd, ci_lo, ci_hi x (alpha, beta, beta/alpha, weight,
    intercept, pr_mm, pr_um, pr_uu)."""
    raw = _f64(raw).reshape(-1, 7)
    with np.errstate(all="ignore"):
        bad = np.isnan(raw).any(axis=1) | np.isnan(raw[:, 1] / raw[:, 0])
    if bad.any():   # abn_analyze sorts with `<`: NaN-free columns only (the reference panics before it gets here)
        raise AbnError(5, f"bootstrap {int(np.flatnonzero(bad)[0])} has no finite fit: no analysis of this table")
    out = np.empty(32)
    _ok(load_library().abn_analyze(_ptr(raw), raw.shape[0], _ptr(out)))
    return out.reshape(4, 8)


def analyze_batch(ctx: "Context", raw, allow_failed_windows=False):
    """analyze() of every window of raw (n_windows, n_boot, 7) in one launch on the device (src/analysis.rs:50-98), with
    the host analysis's bits.  Returns (out (n_windows, 32): mean[8], sd[8], ci_lo[8], ci_hi[8] per window; first_bad
    (n_windows,) int32: the first bootstrap with a NaN row or a NaN beta / alpha, -1 for none).  A window with
    first_bad >= 0 is 32 NaN and raises AbnError(ABN_ERR_NO_FINITE_FIT) unless allow_failed_windows."""
    raw = _f64(raw)
    if raw.ndim != 3 or raw.shape[2] != 7:
        raise ValueError("raw is (n_windows, n_boot, 7)")
    W, B = raw.shape[0], raw.shape[1]
    out, fb = np.empty((W, 32)), np.full(W, -1, dtype=np.int32)
    rc = ctx._L.abn_analyze_batch(ctx._h, _ptr(raw), W, B, _ptr(out), _ptr(fb))
    if not (rc == 5 and allow_failed_windows):  # ABN_ERR_NO_FINITE_FIT: every buffer is filled all the same
        ctx._check(rc)
    return out, fb


class Context:
    """abn_ctx: one HIP device + stream.  `stream`: None = a private stream owned by the context; 0 = the
    device's default (null) stream (torch's current stream unless switched); otherwise a raw hipStream_t."""

    def __init__(self, device: int = 0, stream: int | None = None):
        self._L = load_library()
        h = C.c_void_p()
        if stream is None:
            sp = None
        elif stream == 0:
            sp = C.c_void_p(-1)  # ABN_STREAM_DEFAULT
        else:
            sp = C.c_void_p(stream)
        rc = self._L.abn_init(device, sp, C.byref(h))
        if rc:
            raise AbnError(rc, "abn_init failed (no HIP device? the ABneutral path has no CPU fallback)")
        self._h = h
        self.device = device

    def close(self):
        if getattr(self, "_h", None):
            self._L.abn_shutdown(self._h)
            self._h = None

    def device_info(self):
        """what abn_init read from hipDeviceProp and the persistent-launch geometry derived from it"""
        out = (C.c_int32 * 4)()
        self._check(self._L.abn_device_info(self._h, out))
        return {"compute_units": out[0], "lds_kib_per_cu": out[1], "persistent_wavefronts": out[2],
                "persistent_wavefronts_small": out[3]}

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc:
            raise AbnError(rc, (self._L.abn_last_error(self._h) or b"").decode())

    def _timed(self, entry, *args):
        """the HIP-event ms an entry point (ctx, *args, double*) reports"""
        ms = C.c_double(0.0)
        self._check(entry(self._h, *args, C.byref(ms)))
        return ms.value

    # ---- (1) Problem::cost for M candidates
    def cost_batch(self, pedigree, p_uu0, eqp, eqp_weight, candidates, *, pred=None, resid=None, idx=None,
                   cand_to_boot=None, options: Options | None = None, want_dt=False, want_puu=False):
        ped = _f64(pedigree).reshape(-1, 4)
        cand = _f64(candidates).reshape(-1, 4)
        n, m = ped.shape[0], cand.shape[0]
        cost = np.empty(m)
        dt = np.empty((m, n)) if want_dt else None
        puu = np.empty(m) if want_puu else None
        nb = 0
        if idx is not None:
            idx = _arr(idx, np.uint32).reshape(-1, n)
            nb = idx.shape[0]
            pred, resid = _f64(pred, (n,)), _f64(resid, (n,))
            if cand_to_boot is not None:
                cand_to_boot = _arr(cand_to_boot, np.uint32, m)
        self._check(self._L.abn_cost_batch(self._h, _opt(options), _ptr(ped), n, p_uu0, eqp, eqp_weight, _ptr(cand), m,
                                           _ptr(pred), _ptr(resid), _ptr(idx), _ptr(cand_to_boot), nb, _ptr(cost),
                                           _ptr(dt), _ptr(puu)))
        out = [cost]
        if want_dt:
            out.append(dt)
        if want_puu:
            out.append(puu)
        return out[0] if len(out) == 1 else tuple(out)

    def _fit_batch(self, entry, pedigree, p_uu0, eqp, eqp_weight, simplex0, max_iters, dobs_rows, options, *passes):
        ped = _f64(pedigree).reshape(-1, 4)
        s0 = _f64(simplex0).reshape(-1, 20)
        n, f = ped.shape[0], s0.shape[0]
        d = None if dobs_rows is None else _f64(dobs_rows, (f, n))
        best = np.empty((f, 4))
        info = np.zeros(f, dtype=FIT_INFO_DTYPE)
        self._check(entry(self._h, _opt(options), _ptr(ped), n, p_uu0, eqp, eqp_weight, _ptr(s0), f, _ptr(d), max_iters,
                          _ptr(best), _ptr(info), *passes))
        return best, info

    # ---- Nelder-Mead fits from explicit start simplices
    def fit_batch(self, pedigree, p_uu0, eqp, eqp_weight, simplex0, max_iters, *, dobs_rows=None,
                  options: Options | None = None):
        return self._fit_batch(self._L.abn_fit_batch, pedigree, p_uu0, eqp, eqp_weight, simplex0, max_iters, dobs_rows,
                               options)

    def fit_batch_sweep(self, pedigree, p_uu0, eqp, eqp_weight, simplex0, max_iters, *, dobs_rows=None,
                        options: Options | None = None):
        """fit_batch on the sweep kernel (one pass over the rows per iteration): (best, info, passes over the rows).
        Refused (ABN_ERR_INVALID_ARG) when the pedigree and the options do not route to that kernel."""
        passes = C.c_int64(0)
        best, info = self._fit_batch(self._L.abn_fit_batch_sweep, pedigree, p_uu0, eqp, eqp_weight, simplex0, max_iters,
                                     dobs_rows, options, C.byref(passes))
        return best, info, int(passes.value)

    def gen_boot_indices(self, seed, window, b0, nb, n_rows) -> np.ndarray:
        idx = np.empty((nb, n_rows), dtype=np.uint32)
        self._check(self._L.abn_gen_boot_indices(self._h, seed, window, b0, nb, n_rows, _ptr(idx)))
        return idx

    # ---- (2) ab_neutral::run
    def ab_neutral_run(self, pedigree, p0uu, eqp, eqp_weight, n_starts, *, options: Options | None = None):
        ped = _f64(pedigree).reshape(-1, 4)
        n = ped.shape[0]
        model, pred, resid = np.empty(4), np.empty(n), np.empty(n)
        allm = np.empty((n_starts, 4))
        info = np.zeros(n_starts, dtype=FIT_INFO_DTYPE)
        lse = np.empty(n_starts)
        self._check(self._L.abn_ab_neutral_run(self._h, _opt(options), _ptr(ped), n, p0uu, eqp, eqp_weight, n_starts,
                                               _ptr(model), _ptr(pred), _ptr(resid), _ptr(allm), _ptr(info), _ptr(lse)))
        return model, pred, resid, {"models": allm, "info": info, "lse": lse}

    def select_best(self, pedigree, p0uu, models):
        """src/ab_neutral.rs:83-135: (index, model, pred, resid, lse)"""
        ped = _f64(pedigree).reshape(-1, 4)
        m = _f64(models).reshape(-1, 4)
        n = ped.shape[0]
        k = C.c_int32(-1)
        model, pred, resid, lse = np.empty(4), np.empty(n), np.empty(n), np.empty(m.shape[0])
        self._check(self._L.abn_select_best(self._h, _ptr(ped), n, p0uu, _ptr(m), m.shape[0], C.byref(k), _ptr(model),
                                            _ptr(pred), _ptr(resid), _ptr(lse)))
        return k.value, model, pred, resid, lse

    def bootstrap_rows(self, best):
        """src/boot_model.rs:86-91"""
        b = _f64(best).reshape(-1, 4)
        raw = np.empty((b.shape[0], 7))
        self._check(self._L.abn_bootstrap_rows(self._h, _ptr(b), b.shape[0], _ptr(raw)))
        return raw

    def pairwise_divergence(self, codes):
        """DMatrix::from (src/pedigree.rs:210-261).  codes: (n_samples, n_sites) u8 = status | 0x80 if filtered.
        Returns (diff u64, both u64, dvalue f64), one entry per pair i < j in nested-loop order."""
        codes = _arr(codes, np.uint8)
        n, L = codes.shape
        diff, both, dval = _pair_outputs(n)
        self._check(self._L.abn_pairwise_divergence(self._h, _ptr(codes), n, L, _ptr(diff), _ptr(both), _ptr(dval)))
        return diff, both, dval

    def pairwise_divergence_dev(self, codes_ptr: int, n_samples: int, n_sites: int, diff_ptr: int = 0,
                                both_ptr: int = 0, dvalue_ptr: int = 0) -> float:
        """The same on device-resident buffers (raw device pointers, e.g. torch tensors' data_ptr()): u8 codes
        [n x L] in, u64 diff / both and f64 dvalue [pairs] out (0 = not wanted).  Returns the kernels' HIP-event ms."""
        return self._timed(self._L.abn_pairwise_divergence_dev, _dev(codes_ptr), n_samples, n_sites,
                           _dev(diff_ptr), _dev(both_ptr), _dev(dvalue_ptr))

    def pairwise_divergence_packed(self, packed, n_sites: int):
        """pairwise_divergence on 2-bit packed codes (pack_codes): packed (n_samples, row_stride) u8, n_sites sites per
        sample.  The same (diff, both, dvalue), bit for bit."""
        packed = _arr(packed, np.uint8)
        n, stride = packed.shape
        diff, both, dval = _pair_outputs(n)
        self._check(self._L.abn_pairwise_divergence_packed(self._h, _ptr(packed), n, int(n_sites), stride, _ptr(diff),
                                                           _ptr(both), _ptr(dval)))
        return diff, both, dval

    def pairwise_divergence_packed_dev(self, packed_ptr: int, n_samples: int, n_sites: int, row_stride: int,
                                       diff_ptr: int = 0, both_ptr: int = 0, dvalue_ptr: int = 0) -> float:
        """The same on device-resident buffers: packed rows [n x row_stride] (16-byte aligned) in, u64 diff / both and
        f64 dvalue [pairs] out (0 = not wanted).  Returns the kernels' HIP-event ms."""
        return self._timed(self._L.abn_pairwise_divergence_packed_dev, _dev(packed_ptr), n_samples, n_sites,
                           row_stride, _dev(diff_ptr), _dev(both_ptr), _dev(dvalue_ptr))

    def pairwise_divergence_windows(self, codes, begin, end):
        """pairwise_divergence of the column ranges [begin[w], end[w]) of one (n_samples, row_stride) code matrix in one
        batched call (the window loop of src/cli/metaprofile.rs:50-72).  Returns (diff, both, dvalue), each of shape
        (n_windows, pairs), bit-identical to pairwise_divergence(codes[:, b:e]) per window."""
        codes = _arr(codes, np.uint8)
        n, stride = codes.shape
        b, e = _window_ranges(begin, end)
        W = b.shape[0]
        diff, both, dval = _pair_outputs(n, (W,))
        self._check(self._L.abn_pairwise_divergence_windows(
            self._h, _ptr(codes), n, stride, _ptr(b), _ptr(e), W, _ptr(diff), _ptr(both), _ptr(dval)))
        return diff, both, dval

    def pairwise_divergence_windows_dev(self, codes_ptr: int, n_samples: int, row_stride: int, begin, end,
                                        diff_ptr: int = 0, both_ptr: int = 0, dvalue_ptr: int = 0) -> float:
        """The same on device-resident buffers: u8 codes [n x row_stride] in, u64 diff / both and f64 dvalue
        [n_windows x pairs] out (0 = not wanted); begin / end are host arrays.  Returns the kernels' HIP-event ms."""
        b, e = _window_ranges(begin, end)
        return self._timed(self._L.abn_pairwise_divergence_windows_dev, _dev(codes_ptr), n_samples, row_stride,
                           _ptr(b), _ptr(e), b.shape[0], _dev(diff_ptr), _dev(both_ptr), _dev(dvalue_ptr))

    def pairwise_divergence_windows_packed(self, packed, n_sites: int, begin, end):
        """pairwise_divergence_windows on 2-bit packed codes (pack_codes): packed (n_samples, row_stride) u8 with n_sites
        sites per sample; windows [begin[w], end[w]) in sites, at any site.  Returns (diff, both, dvalue), each of shape
        (n_windows, pairs), bit-identical to pairwise_divergence_windows on the unpacked codes."""
        packed = _arr(packed, np.uint8)
        n, stride = packed.shape
        b, e = _window_ranges(begin, end)
        W = b.shape[0]
        diff, both, dval = _pair_outputs(n, (W,))
        self._check(self._L.abn_pairwise_divergence_windows_packed(
            self._h, _ptr(packed), n, int(n_sites), stride, _ptr(b), _ptr(e), W, _ptr(diff), _ptr(both), _ptr(dval)))
        return diff, both, dval

    def pairwise_divergence_windows_packed_dev(self, packed_ptr: int, n_samples: int, n_sites: int, row_stride: int,
                                               begin, end, diff_ptr: int = 0, both_ptr: int = 0,
                                               dvalue_ptr: int = 0) -> float:
        """The same on device-resident buffers: packed rows [n x row_stride] (16-byte aligned) in, u64 diff / both and
        f64 dvalue [n_windows x pairs] out (0 = not wanted); begin / end are host arrays.  Returns the kernels'
        HIP-event ms."""
        b, e = _window_ranges(begin, end)
        return self._timed(self._L.abn_pairwise_divergence_windows_packed_dev, _dev(packed_ptr), n_samples,
                           n_sites, row_stride, _ptr(b), _ptr(e), b.shape[0], _dev(diff_ptr), _dev(both_ptr),
                           _dev(dvalue_ptr))

    def pairwise_transitions_packed(self, packed, n_sites: int):
        """The 3 x 3 state transitions of every pair on 2-bit packed codes (pack_codes): uint64 (pairs, 3, 3), entry
        [p, x, y] = the sites both samples of pair p = (a, b), a < b, keep with status x in a and y in b (0 = U, 1 = I,
        2 = M).  Its sum is pairwise_divergence_packed's both, its |x - y|-weighted sum the diff."""
        packed = _arr(packed, np.uint8)
        n, stride = packed.shape
        table = _pair_tables(n)
        self._check(self._L.abn_pairwise_transitions_packed(self._h, _ptr(packed), n, int(n_sites), stride, _ptr(table)))
        return table

    def pairwise_transitions_packed_dev(self, packed_ptr: int, n_samples: int, n_sites: int, row_stride: int,
                                        table_ptr: int) -> float:
        """The same on device-resident buffers: packed rows [n x row_stride] (16-byte aligned) in, u64 table
        [pairs x 9] out.  Returns the kernels' HIP-event ms."""
        return self._timed(self._L.abn_pairwise_transitions_packed_dev, _dev(packed_ptr), n_samples, n_sites,
                           row_stride, _dev(table_ptr))

    def pairwise_transitions_windows_packed(self, packed, n_sites: int, begin, end):
        """pairwise_transitions_packed of the column ranges [begin[w], end[w]) (in sites, at any site) of one packed
        matrix in one batched call: uint64 (n_windows, pairs, 3, 3); an empty window's table is zero."""
        packed = _arr(packed, np.uint8)
        n, stride = packed.shape
        b, e = _window_ranges(begin, end)
        table = _pair_tables(n, (b.shape[0],))
        self._check(self._L.abn_pairwise_transitions_windows_packed(
            self._h, _ptr(packed), n, int(n_sites), stride, _ptr(b), _ptr(e), b.shape[0], _ptr(table)))
        return table

    def pairwise_transitions_windows_packed_dev(self, packed_ptr: int, n_samples: int, n_sites: int, row_stride: int,
                                                begin, end, table_ptr: int) -> float:
        """The same on device-resident buffers: packed rows [n x row_stride] (16-byte aligned) in, u64 table
        [n_windows x pairs x 9] out; begin / end are host arrays.  Returns the kernels' HIP-event ms."""
        b, e = _window_ranges(begin, end)
        return self._timed(self._L.abn_pairwise_transitions_windows_packed_dev, _dev(packed_ptr), n_samples,
                           n_sites, row_stride, _ptr(b), _ptr(e), b.shape[0], _dev(table_ptr))

    def block_counts(self, seed: int, group_id, group_begin, group_end, n_replicates: int, n_blocks: int) -> np.ndarray:
        """The block bootstrap's counts, made on the device (abn_block_counts): uint8 (G, n_replicates + 1, n_blocks).
        Row r < n_replicates of group g is the histogram of T_g draws from the group's blocks [group_begin[g],
        group_end[g]), a function of (seed, group_id[g], r) alone; the last row is the identity row of ones; zero
        outside a group's range."""
        gid, gb, ge = _block_groups(group_begin, group_end, group_id)
        counts = _block_counts_array(gb.shape[0], n_replicates, n_blocks)
        self._check(self._L.abn_block_counts(self._h, int(seed), gb.shape[0], _ptr(gid), _ptr(gb), _ptr(ge),
                                             int(n_replicates), int(n_blocks), _ptr(counts)))
        return counts

    def block_resample(self, group_begin, group_end, counts, both, diff, level_sum_kept, kept):
        """Every row's sums over its group's blocks (abn_block_resample), exact: counts uint8 (G, rows, T) — drawn by
        block_counts, or any weights 0 .. 127 such as a jackknife's —, both / diff uint64 (T, pairs), level_sum_kept /
        kept (n, T).  Returns {both, diff, dvalue: (G, rows, pairs); level, kept: (G, rows, n)}."""
        a = _block_arguments(group_begin, group_end, counts, both, diff, level_sum_kept, kept)
        out = _block_outputs(*a["dims"])
        self._check(self._L.abn_block_resample(self._h, *_block_pointers(a, out)))
        return out

    def block_resample_dev(self, group_begin, group_end, rows_per_group: int, counts_ptr: int, n_blocks: int, n_pairs: int,
                           n_samples: int, both_ptr: int, diff_ptr: int, level_ptr: int, kept_ptr: int, both_out_ptr: int = 0,
                           diff_out_ptr: int = 0, dvalue_out_ptr: int = 0, level_out_ptr: int = 0,
                           kept_out_ptr: int = 0) -> np.ndarray:
        """block_resample on device-resident buffers (raw device pointers; an output of 0 is not wanted).  Returns the
        HIP-event ms of counts (0 here), digits, product, finish, levels."""
        _, gb, ge = _block_groups(group_begin, group_end)
        ms = np.zeros(5)
        ptr = [_dev(p) for p in (both_ptr, diff_ptr, level_ptr, kept_ptr, both_out_ptr, diff_out_ptr, dvalue_out_ptr,
                                 level_out_ptr, kept_out_ptr)]
        self._check(self._L.abn_block_resample_dev(self._h, gb.shape[0], _ptr(gb), _ptr(ge), int(rows_per_group),
                                                   _dev(counts_ptr), int(n_blocks), int(n_pairs), int(n_samples), *ptr,
                                                   _ptr(ms)))
        return ms

    def analyze_batch_dev(self, raw_ptr: int, n_windows: int, n_boot: int, out_ptr: int, first_bad_ptr: int = 0,
                          allow_failed_windows=False) -> float:
        """analyze_batch on device-resident buffers (raw device pointers): f64 raw [n_windows x n_boot x 7] in, f64 out
        [n_windows x 32] and i32 first_bad [n_windows] (0 = not wanted) out.  Returns the kernel's HIP-event ms."""
        ms = C.c_double(0.0)
        rc = self._L.abn_analyze_batch_dev(self._h, _dev(raw_ptr), n_windows, n_boot, _dev(out_ptr), _dev(first_bad_ptr),
                                           C.byref(ms))
        if not (rc == 5 and allow_failed_windows):
            self._check(rc)
        return ms.value

    def _parse(self, entry, text, skip_lines, slab_bytes, contexts):
        """(mask, Sites) of one of the two parse entry points"""
        text = bytes(text)
        mask = _context_mask(contexts)
        p = SitesParams(slab_bytes, skip_lines, 0 if mask == 1 else mask)
        h = C.c_void_p()
        self._check(entry(self._h, text, len(text), C.byref(p), C.byref(h)))
        return mask, Sites(self, h)

    def parse_sites(self, text: bytes, *, skip_lines: int = 1, slab_bytes: int = 0, contexts=("CG",)):
        """MethylationSite::from_methylome_file_line (src/methylation_site.rs:146-362) for every line of a methylome
        file's text from line skip_lines on, on the device.  Returns (sites, deferred): sites = a dict of arrays over the
        accepted sites in file order (line, chromosome, start, end, strand, posteriormax, status, status_flag, meth_lvl;
        n_lines and kernel_ms beside them); deferred = a dict of line, offset, length of the lines the device leaves to
        the host's parser (an f64 field it cannot be certain of, a line beyond its staging limit).  contexts: the
        methylation contexts whose lines are sites (names of CONTEXTS, or the mask); with any other value than CG alone
        sites gains `context`, every site's code (0 CG, 1 CHG, 2 CHH, 3 a row without one)."""
        mask, s = self._parse(self._L.abn_sites_parse, text, skip_lines, slab_bytes, contexts)
        try:
            sites, deferred = s.fetch(), s.deferred()
            sites.update(s.info())
            del sites["n_sites"], sites["n_deferred"]
            if mask != 1:
                sites["context"] = s.contexts()
            return sites, deferred
        finally:
            s.close()

    def parse_sites_resident(self, text: bytes, *, skip_lines: int = 1, slab_bytes: int = 0, contexts=("CG",)) -> "Sites":
        """parse_sites with the records left on the device (abn_sites_parse_dev): a Sites handle for Windows.from_parsed.
        Its deferred() lines are for the caller's parser; those it accepts go back in with insert(), once.  A handle of
        several contexts gives one handle per context with split()."""
        return self._parse(self._L.abn_sites_parse_dev, text, skip_lines, slab_bytes, contexts)[1]

    def choose_genes(self, genes: "Genes", site_offset, chromosome, start, end, strand, *, cutoff,
                     cutoff_gene_length=False):
        """The gene of every site (the loop of Windows::extract, src/windows.rs:325-338, with is_in_gene / find_gene and
        the last_gene cache) for n_samples methylomes, on the device.  site_offset (n_samples + 1,) int64; per site
        (concatenated over the samples, file order) chromosome int32, start, end uint32, strand uint8 (0 +, 1 -, 2
        unknown).  Returns (gene_start, gene_end, flags, kernel_ms): what Windows(...) takes, and the three kernels' ms."""
        off, u = _site_arrays(site_offset, chromosome, start, end, strand)
        S = int(off[-1])
        gs, ge, fl = np.zeros(S, dtype=np.uint32), np.zeros(S, dtype=np.uint32), np.zeros(S, dtype=np.uint8)
        ms = np.zeros(3)
        rule = GeneRule(cutoff, 1 if cutoff_gene_length else 0)
        self._check(self._L.abn_genes_choose(genes._h, C.byref(rule), off.shape[0] - 1, _ptr(off), *map(_ptr, u),
                                             _ptr(gs), _ptr(ge), _ptr(fl), _ptr(ms)))
        return gs, ge, fl, ms

    def common_sites(self, site_offset, chromosome, start, end, strand):
        """The sites every sample shares, by key (chromosome, start, end, strand), on the device (abn_sites_common: lifts
        the assumption of src/pedigree.rs:240).  Arguments as choose_genes.  Returns (keep uint8 (S,), n_common): keep marks
        every sample's common sites, n_common of them in each.  AbnError when a sample is not well ordered (a chromosome in
        two runs, a key not above the one before it) or the samples' common sites come in different orders."""
        off, u = _site_arrays(site_offset, chromosome, start, end, strand)
        keep = np.zeros(int(off[-1]), dtype=np.uint8)
        n_common = C.c_int64(-1)
        self._check(self._L.abn_sites_common(self._h, off.shape[0] - 1, _ptr(off), *map(_ptr, u), _ptr(keep),
                                             C.byref(n_common)))
        return keep, n_common.value

    def sort_sites(self, chromosome, start, end, strand):
        """The stable permutation of one sample's keys into canonical order — ascending chromosome, start, end, strand — on
        the device (abn_sites_sort_keys).  Returns (order int64 (n,), info): info = {sites, descents, equal, passes} as
        Sites.sort_info.  AbnError for a chromosome outside 0..257 or a strand above 2."""
        n = np.asarray(chromosome).reshape(-1).shape[0]
        _, u = _site_arrays([0, n], chromosome, start, end, strand)
        order, info = np.zeros(n, dtype=np.int64), np.zeros(4, dtype=np.int64)
        self._check(self._L.abn_sites_sort_keys(self._h, n, *map(_ptr, u), _ptr(order), _ptr(info)))
        return order, _sort_info(info)

    def union_sites(self, site_offset, chromosome, start, end, strand):
        """The union of the samples' sites, by key (chromosome, start, end, strand), on the device (abn_sites_union: the
        per-pair comparison of src/pedigree.rs:240-254 for samples that hold different sites).  Arguments as common_sites.
        Returns (dest uint32 (S,), n_union): every site's rank in the union order, n_union distinct keys.  AbnError when a
        sample is not well ordered or its chromosomes come in another order than the union's."""
        off, u = _site_arrays(site_offset, chromosome, start, end, strand)
        dest = np.zeros(int(off[-1]), dtype=np.uint32)
        n_union = C.c_int64(-1)
        self._check(self._L.abn_sites_union(self._h, off.shape[0] - 1, _ptr(off), *map(_ptr, u), _ptr(dest),
                                            C.byref(n_union)))
        return dest, n_union.value

    def choose_genes_dev(self, genes: "Genes", site_offset, chromosome_ptr: int, start_ptr: int, end_ptr: int,
                         strand_ptr: int, gene_start_ptr: int, gene_end_ptr: int, flags_ptr: int, *, cutoff,
                         cutoff_gene_length=False) -> np.ndarray:
        """choose_genes on device-resident arrays (raw device pointers; site_offset stays a host array).  Returns the
        three kernels' HIP-event ms."""
        off = _arr(site_offset, np.int64)
        ms = np.zeros(3)
        rule = GeneRule(cutoff, 1 if cutoff_gene_length else 0)
        self._check(self._L.abn_genes_choose_dev(genes._h, C.byref(rule), off.shape[0] - 1, _ptr(off),
                                                 *(_dev(p) for p in (chromosome_ptr, start_ptr, end_ptr, strand_ptr,
                                                                     gene_start_ptr, gene_end_ptr, flags_ptr)), _ptr(ms)))
        return ms

    # ---- (3) boot_model::run
    def boot_model_run(self, pedigree, model, pred, resid, p0uu, eqp, eqp_weight, n_boot, *,
                       options: Options | None = None):
        ped = _f64(pedigree).reshape(-1, 4)
        n = ped.shape[0]
        raw = np.empty((n_boot, 7))
        info = np.zeros(n_boot, dtype=FIT_INFO_DTYPE)
        self._check(self._L.abn_boot_model_run(self._h, _opt(options), _ptr(ped), n, _ptr(_f64(model, (4,))),
                                               _ptr(_f64(pred, (n,))), _ptr(_f64(resid, (n,))), p0uu, eqp, eqp_weight,
                                               n_boot, _ptr(raw), _ptr(info)))
        return raw, info
