"""The FFI layer of the binding: status names, structs and record dtypes of include/abneutral.h, the one table of its
prototypes, the loaders of the two libraries, and the helpers every handle family's module casts and allocates with."""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

import numpy as np

from . import build as _build

PKG = Path(__file__).resolve().parent
LIB_PATH = PKG / "libabneutral_hip.so"
if os.environ.get("ABNEUTRAL_HIP_LIB"):  # development aid (scripts/flag_variants.py): another build of the same library
    LIB_PATH = Path(os.environ["ABNEUTRAL_HIP_LIB"])

ABN_OK = 0
STATUS_NAMES = {
    0: "ABN_OK",
    1: "ABN_ERR_INVALID_ARG",
    2: "ABN_ERR_BAD_PEDIGREE",
    3: "ABN_ERR_NO_DEVICE",
    4: "ABN_ERR_HIP",
    5: "ABN_ERR_NO_FINITE_FIT",
    6: "ABN_ERR_STATE",
}
FIT_CONVERGED, FIT_MAX_ITERS, FIT_NONFINITE, FIT_TARGET = 0, 1, 2, 3
KERNEL_NAMES = {0: "none", 1: "speculative", 2: "resident", 3: "persistent", 4: "stream", 5: "two_pass",
                6: "stream_sweep"}

FIT_INFO_DTYPE = np.dtype(
    [("best_cost", "<f8"), ("iters", "<i4"), ("evals", "<i4"), ("status", "<i4"), ("lanes", "<i4")]
)


class Options(C.Structure):
    _fields_ = [
        ("seed", C.c_uint64),
        ("lanes_per_chain", C.c_int32),
        ("strict_order", C.c_int32),
        ("shrink_on_failed_contraction", C.c_int32),
        ("max_iters_start", C.c_int32),
        ("max_iters_boot", C.c_int32),
        ("stream_mode", C.c_int32),
        ("sd_tolerance", C.c_double),
        ("window_groups", C.c_int32),
        ("no_fixed_point_skip", C.c_int32),
    ]


class WindowsParams(C.Structure):
    """abn_windows_params: arguments::Windows and the window counts of Windows::new (src/windows.rs:28-44)"""
    _fields_ = [
        ("cutoff", C.c_uint32),
        ("step", C.c_uint32),
        ("size", C.c_uint32),
        ("absolute", C.c_int32),
        ("n_upstream", C.c_int32),
        ("n_gene", C.c_int32),
        ("n_downstream", C.c_int32),
    ]


class GeneRule(C.Structure):
    """abn_gene_rule: the two arguments is_in_gene and find_gene read"""
    _fields_ = [
        ("cutoff", C.c_uint32),
        ("cutoff_gene_length", C.c_int32),
    ]


class SitesParams(C.Structure):
    """abn_sites_params: the slab size of abn_sites_parse (0: the default) and the leading lines it does not parse"""
    _fields_ = [
        ("slab_bytes", C.c_int64),
        ("skip_lines", C.c_int32),
        ("contexts", C.c_int32),
    ]


class AbnError(RuntimeError):
    def __init__(self, status: int, detail: str = ""):
        self.status = status
        super().__init__(f"{STATUS_NAMES.get(status, status)}: {detail}")


def _ok(rc, detail=""):
    """the status of a call that has no context to ask for the error's text"""
    if rc:
        raise AbnError(rc, detail)


def _prototypes():
    """name -> (restype, [argtypes]) of every symbol include/abneutral.h declares, in the header's order
    (tests/test_abi.py holds each entry to its declaration).  A handle and a device address are vp, a record array of
    abn_fit_info too."""
    ci, i32, i64, u32, u64, f64 = C.c_int, C.c_int32, C.c_int64, C.c_uint32, C.c_uint64, C.c_double
    vp, text = C.c_void_p, C.c_char_p
    cip, i32p, i64p, u8p, u32p, u64p, dp, vpp = (C.POINTER(t) for t in (ci, i32, i64, C.c_uint8, u32, u64, f64, vp))
    op, wp, gp, sp = (C.POINTER(t) for t in (Options, WindowsParams, GeneRule, SitesParams))
    return {
        "abn_default_options": (None, [op]),
        "abn_device_count": (ci, [cip]),
        "abn_init": (ci, [ci, vp, vpp]),
        "abn_shutdown": (ci, [vp]),
        "abn_device_info": (ci, [vp, i32p]),
        "abn_last_error": (text, [vp]),
        "abn_status_string": (text, [ci]),
        "abn_version": (ci, []),
        "abn_reduction_tree": (ci, [op, dp, i32, i32p]),
        "abn_cost_batch": (ci, [vp, op, dp, i32, f64, f64, f64, dp, i64, dp, dp, u32p, u32p, i64, dp, dp, dp]),
        "abn_fit_batch": (ci, [vp, op, dp, i32, f64, f64, f64, dp, i64, dp, i32, dp, vp]),
        "abn_fit_batch_sweep": (ci, [vp, op, dp, i32, f64, f64, f64, dp, i64, dp, i32, dp, vp, i64p]),
        "abn_gen_start_simplices": (ci, [u64, u32, i32, f64, dp]),
        "abn_gen_boot_simplices": (ci, [u64, u32, u32, i64, dp, dp]),
        "abn_gen_boot_indices": (ci, [vp, u64, u32, u32, i64, i32, u32p]),
        "abn_ab_neutral_run": (ci, [vp, op, dp, i32, f64, f64, f64, i32, dp, dp, dp, dp, vp, dp]),
        "abn_select_best": (ci, [vp, dp, i32, f64, dp, i32, i32p, dp, dp, dp, dp]),
        "abn_bootstrap_rows": (ci, [vp, dp, i64, dp]),
        "abn_boot_model_run": (ci, [vp, op, dp, i32, dp, dp, dp, f64, f64, f64, i32, dp, vp]),
        "abn_analyze": (ci, [dp, i64, dp]),
        "abn_analyze_batch": (ci, [vp, dp, i32, i64, dp, i32p]),
        "abn_analyze_batch_dev": (ci, [vp, vp, i32, i64, vp, vp, dp]),
        "abn_pairwise_divergence": (ci, [vp, u8p, i32, i64, u64p, u64p, dp]),
        "abn_pairwise_divergence_dev": (ci, [vp, vp, i32, i64, vp, vp, vp, dp]),
        "abn_pairwise_divergence_windows": (ci, [vp, u8p, i32, i64, i64p, i64p, i32, u64p, u64p, dp]),
        "abn_pairwise_divergence_windows_dev": (ci, [vp, vp, i32, i64, i64p, i64p, i32, vp, vp, vp, dp]),
        "abn_packed_row_stride": (i64, [i64]),
        "abn_pack_codes": (ci, [u8p, i32, i64, i64, u8p, i64]),
        "abn_unpack_codes": (ci, [u8p, i32, i64, i64, u8p, i64]),
        "abn_pairwise_divergence_packed": (ci, [vp, u8p, i32, i64, i64, u64p, u64p, dp]),
        "abn_pairwise_divergence_packed_dev": (ci, [vp, vp, i32, i64, i64, vp, vp, vp, dp]),
        "abn_pairwise_divergence_windows_packed": (ci, [vp, u8p, i32, i64, i64, i64p, i64p, i32, u64p, u64p, dp]),
        "abn_pairwise_divergence_windows_packed_dev": (ci, [vp, vp, i32, i64, i64, i64p, i64p, i32, vp, vp, vp, dp]),
        "abn_pairwise_transitions_packed": (ci, [vp, u8p, i32, i64, i64, u64p]),
        "abn_pairwise_transitions_packed_dev": (ci, [vp, vp, i32, i64, i64, vp, dp]),
        "abn_pairwise_transitions_windows_packed": (ci, [vp, u8p, i32, i64, i64, i64p, i64p, i32, u64p]),
        "abn_pairwise_transitions_windows_packed_dev": (ci, [vp, vp, i32, i64, i64, i64p, i64p, i32, vp, dp]),
        "abn_packed_census_windows": (ci, [vp, u8p, i32, i64, i64, i64p, i64p, i32, u64p]),
        "abn_packed_census_windows_dev": (ci, [vp, vp, i32, i64, i64, i64p, i64p, i32, vp, dp]),
        "abn_packed_region_states": (ci, [vp, u8p, i32, i64, i64, i64p, i64p, i64, i32p, i64, i64, i64, i64, i64, i64, u8p]),
        "abn_packed_region_states_dev": (ci, [vp, vp, i32, i64, i64, i64p, i64p, i64, i32p, i64, i64, i64, i64, i64, i64, vp,
                                              dp]),
        "abn_windows_create": (ci, [vp, wp, i32, i64p, u32p, u32p, u32p, u8p, u8p, dp, vpp]),
        "abn_windows_destroy": (ci, [vp]),
        "abn_windows_info": (ci, [vp, i32p, i64p, i64p]),
        "abn_windows_stats": (ci, [vp, i64p, dp, dp, i64p]),
        "abn_windows_layout": (ci, [vp, i64p, i64p, i32p]),
        "abn_windows_packed": (ci, [vp, u8p]),
        "abn_windows_packed_device_ptr": (ci, [vp, vpp]),
        "abn_windows_pairwise": (ci, [vp, u64p, u64p, dp]),
        "abn_genes_create": (ci, [vp, i32, i32p, i32p, i64p, u32p, u32p, u8p, vpp]),
        "abn_genes_destroy": (ci, [vp]),
        "abn_genes_choose": (ci, [vp, gp, i32, i64p, i32p, u32p, u32p, u8p, u32p, u32p, u8p, dp]),
        "abn_genes_choose_dev": (ci, [vp, gp, i32, i64p, vp, vp, vp, vp, vp, vp, vp, dp]),
        "abn_windows_create_sites": (ci, [vp, wp, vp, gp, i32, i64p, i32p, u32p, u32p, u8p, u8p, dp, vpp]),
        "abn_sites_parse": (ci, [vp, text, i64, sp, vpp]),
        "abn_sites_destroy": (ci, [vp]),
        "abn_sites_info": (ci, [vp, i64p, i64p, i64p, dp]),
        "abn_sites_fetch": (ci, [vp, i64p, i32p, u32p, u32p, u8p, dp, u8p, u8p, dp]),
        "abn_sites_deferred": (ci, [vp, i64p, i64p, i64p]),
        "abn_sites_parse_dev": (ci, [vp, text, i64, sp, vpp]),
        "abn_sites_flagged": (ci, [vp, i64p, i64p]),
        "abn_sites_insert": (ci, [vp, i64, i64p, i32p, u32p, u32p, u8p, dp, u8p, dp]),
        "abn_sites_context": (ci, [vp, i32p, u8p]),
        "abn_sites_insert_ctx": (ci, [vp, i64, i64p, i32p, u32p, u32p, u8p, dp, u8p, dp, u8p]),
        "abn_sites_split": (ci, [vp, vpp]),
        "abn_sites_split_ms": (ci, [vp, dp]),
        "abn_sites_sort": (ci, [vp, vpp]),
        "abn_sites_sort_order": (ci, [vp, i64p, i64p]),
        "abn_sites_sort_info": (ci, [vp, i64p, dp]),
        "abn_sites_sort_keys": (ci, [vp, i64, i32p, u32p, u32p, u8p, i64p, i64p]),
        "abn_sites_sort_keys_dev": (ci, [vp, i64, vp, vp, vp, vp, vp, i64p, dp]),
        "abn_sites_dedup": (ci, [vp, ci, vpp]),
        "abn_sites_dedup_order": (ci, [vp, i64p, i64p]),
        "abn_sites_dedup_info": (ci, [vp, i64p, dp]),
        "abn_sites_dedup_keys": (ci, [vp, i64, i32p, u32p, u32p, u8p, dp, u8p, ci, i64p, i64p]),
        "abn_sites_dedup_keys_dev": (ci, [vp, i64, vp, vp, vp, vp, vp, vp, ci, vp, i64p, dp]),
        "abn_windows_create_parsed": (ci, [vp, wp, vp, gp, f64, i32, vpp, vpp]),
        "abn_windows_merge_ms": (ci, [vp, dp]),
        "abn_codes_create_parsed": (ci, [vp, f64, i32, vpp, vpp]),
        "abn_codes_destroy": (ci, [vp]),
        "abn_codes_info": (ci, [vp, i32p, i64p, i64p, i32p]),
        "abn_codes_stats": (ci, [vp, i64p, dp, i64p]),
        "abn_codes_packed": (ci, [vp, u8p]),
        "abn_codes_packed_device_ptr": (ci, [vp, vpp]),
        "abn_codes_pairwise": (ci, [vp, u64p, u64p, dp]),
        "abn_codes_transitions": (ci, [vp, u64p]),
        "abn_codes_kernel_ms": (ci, [vp, dp]),
        "abn_sites_common": (ci, [vp, i32, i64p, i32p, u32p, u32p, u8p, u8p, i64p]),
        "abn_sites_common_dev": (ci, [vp, i32, i64p, vp, vp, vp, vp, vp, i64p]),
        "abn_windows_create_aligned": (ci, [vp, wp, vp, gp, f64, i32, vpp, vpp]),
        "abn_codes_create_aligned": (ci, [vp, f64, i32, vpp, vpp]),
        "abn_windows_common": (ci, [vp, i64p, i64p, dp]),
        "abn_codes_common": (ci, [vp, i64p, i64p, dp]),
        "abn_sites_union": (ci, [vp, i32, i64p, i32p, u32p, u32p, u8p, u32p, i64p]),
        "abn_sites_union_dev": (ci, [vp, i32, i64p, vp, vp, vp, vp, vp, i64p]),
        "abn_windows_create_union": (ci, [vp, wp, vp, gp, f64, i32, vpp, vpp]),
        "abn_codes_create_union": (ci, [vp, f64, i32, vpp, vpp]),
        "abn_windows_union": (ci, [vp, i64p, i64p, dp]),
        "abn_codes_union": (ci, [vp, i64p, i64p, dp]),
        "abn_tiles_create": (ci, [vp, f64, i32, i32, vpp, vpp]),
        "abn_tiles_destroy": (ci, [vp]),
        "abn_tiles_info": (ci, [vp, i32p, i64p, i64p, i32p, i64p]),
        "abn_tiles_runs": (ci, [vp, i32p, i64p, i64p, u32p]),
        "abn_tiles_set_intervals": (ci, [vp, i64, i32p, i64p, i64p]),
        "abn_tiles_set_fixed": (ci, [vp, i64, i64]),
        "abn_tiles_intervals": (ci, [vp, i32p, i64p, i64p]),
        "abn_tiles_layout": (ci, [vp, i64p, i64p]),
        "abn_tiles_stats": (ci, [vp, i64p, dp, i64p]),
        "abn_tiles_pairwise": (ci, [vp, u64p, u64p, dp]),
        "abn_tiles_transitions": (ci, [vp, u64p]),
        "abn_tiles_kernel_ms": (ci, [vp, dp]),
        "abn_tiles_set_pools": (ci, [vp, i64, i32p, i64p, i64p, i32p, i64]),
        "abn_tiles_pool_segments": (ci, [vp, i64p, i32p, i32p, i64p, i64p, i64p, i64p]),
        "abn_tiles_pool_columns": (ci, [vp, i64p]),
        "abn_tiles_pool_kernel_ms": (ci, [vp, dp]),
        "abn_block_counts": (ci, [vp, u64, i32, u32p, i64p, i64p, i64, i64, u8p]),
        "abn_block_counts_host": (ci, [u64, i32, u32p, i64p, i64p, i64, i64, u8p, text, i32]),
        "abn_block_resample": (ci, [vp, i32, i64p, i64p, i64, u8p, i64, i64, i32, u64p, u64p, dp, i64p, u64p, u64p, dp,
                                    dp, i64p]),
        "abn_block_resample_dev": (ci, [vp, i32, i64p, i64p, i64, vp, i64, i64, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp,
                                        dp]),
        "abn_block_resample_host": (ci, [i32, i64p, i64p, i64, u8p, i64, i64, i32, u64p, u64p, dp, i64p, u64p, u64p, dp,
                                         dp, i64p, text, i32]),
        "abn_tiles_block_bootstrap": (ci, [vp, u64, i64, u64p, u64p, dp, dp, i64p]),
        "abn_tiles_block_groups": (ci, [vp, i64p, i64p, i64p, i64p]),
        "abn_tiles_block_ms": (ci, [vp, dp]),
        "abn_tiles_region_states": (ci, [vp, i64, i64, i64, i64, i32p, i32, vpp]),
        "abn_regions_destroy": (ci, [vp]),
        "abn_regions_info": (ci, [vp, i32p, i64p, i64p, i32p]),
        "abn_regions_layout": (ci, [vp, i64p, i64p]),
        "abn_regions_order": (ci, [vp, i32p]),
        "abn_regions_packed": (ci, [vp, u8p]),
        "abn_regions_packed_device_ptr": (ci, [vp, vpp]),
        "abn_regions_census": (ci, [vp, u64p]),
        "abn_regions_pairwise": (ci, [vp, u64p, u64p, dp]),
        "abn_regions_transitions": (ci, [vp, u64p]),
        "abn_regions_kernel_ms": (ci, [vp, dp]),
        "abn_plan_create": (ci, [vp, op, dp, i32, i32, i32, i32, u32, u32, vpp]),
        "abn_plan_destroy": (ci, [vp]),
        "abn_plan_set_window_ids": (ci, [vp, u32p]),
        "abn_plan_set_windows": (ci, [vp, dp, dp, dp, dp]),
        "abn_plan_run": (ci, [vp]),
        "abn_plan_run_phase": (ci, [vp, i32]),
        "abn_plan_sync": (ci, [vp]),
        "abn_plan_tail_handed": (ci, [vp, i64p]),
        "abn_plan_set_early_bootstraps": (ci, [vp, i32]),
        "abn_plan_early_bootstraps": (ci, [vp, i32p]),
        "abn_plan_set_stream_sweep": (ci, [vp, i32]),
        "abn_plan_stream_sweep": (ci, [vp, i64p]),
        "abn_plan_kernel_ms": (ci, [vp, dp]),
        "abn_plan_raw_device_ptr": (ci, [vp, vpp]),
        "abn_plan_bind_raw": (ci, [vp, vp]),
        "abn_plan_download": (ci, [vp, dp, dp, dp, dp, vp, vp, i32p]),
        "abn_plan_analyze": (ci, [vp, dp, i32p]),
        "abn_plan_failed_windows": (ci, [vp, i32p]),
        "abn_plan_counters": (ci, [vp, i64p]),
        "abn_plan_device_bytes": (ci, [vp, i64p]),
        "abn_plan_last_kernels": (ci, [vp, i32p]),
        "abn_multi_create": (ci, [i32p, i32, op, dp, i32, i32, i32, i32, vpp]),
        "abn_multi_destroy": (ci, [vp]),
        "abn_multi_last_error": (text, [vp]),
        "abn_multi_set_window_ids": (ci, [vp, u32p]),
        "abn_multi_set_stream_sweep": (ci, [vp, i32]),
        "abn_multi_set_windows": (ci, [vp, dp, dp, dp, dp]),
        "abn_multi_run": (ci, [vp]),
        "abn_multi_sync": (ci, [vp]),
        "abn_multi_shard": (ci, [vp, i32, i32p]),
        "abn_multi_plan_shard": (ci, [i32, i32, i32, i32, i32p]),
        "abn_multi_kernel_ms": (ci, [vp, i32, dp]),
        "abn_multi_raw_device_ptr": (ci, [vp, i32, vpp]),
        "abn_multi_download": (ci, [vp, dp, dp, dp, dp, vp, vp, i32p]),
        "abn_multi_analyze": (ci, [vp, dp, i32p]),
        "abn_multi_counters": (ci, [vp, i64p]),
        "abn_multi_rccl_available": (ci, [cip]),
        "abn_sim_thresholds": (ci, [f64, f64, f64, f64, i32, i32p, i32p, u64p, text, i32]),
        "abn_sim_grid": (ci, [vp, i64, i32p]),
        "abn_sim_codes": (ci, [vp, u64, i32, i32p, u64p, u8p, i64, u8p, i64]),
        "abn_sim_codes_dev": (ci, [vp, u64, i32, i32p, u64p, u8p, i64, vp, i64, dp]),
        "abn_sim_pedigree": (ci, [vp, u64, i32, i32p, i32p, u64p, u8p, i64, dp, dp, dp]),
        "abn_sim_obs_thresholds": (ci, [dp, dp, u64p, text, i32]),
        "abn_sim_observe": (ci, [vp, u64, i32, i32p, u64p, i64, u8p, i64, u8p, i64]),
        "abn_sim_observe_dev": (ci, [vp, u64, i32, i32p, u64p, i64, vp, i64, vp, i64, dp]),
        "abn_sim_study": (ci, [vp, u64, i32, i32p, i32p, u64p, u8p, u64p, i64, i32, dp, dp, dp, u64p, dp]),
    }


PROTOTYPES = _prototypes()
EXPORTED_SYMBOLS = list(PROTOTYPES)  # every symbol include/abneutral.h declares (checked by tests/test_abi.py)

_lib = None


def use_library(path):
    """Bind another build of the same library from the next load_library() on (scripts/stamps.py, stream_variants.py)"""
    global LIB_PATH, _lib
    LIB_PATH, _lib = Path(path), None


def load_library(build_if_missing: bool = False) -> C.CDLL:
    """Load libabneutral_hip.so.  Raises (never falls back) when the HIP library is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not LIB_PATH.exists():
        if build_if_missing:
            _build.build_hip()
        else:
            raise FileNotFoundError(
                f"{LIB_PATH} is missing: build it with `python -m alphabeta_rs_amd.build` "
                "(the ABneutral path has no CPU fallback)"
            )
    L = C.CDLL(str(LIB_PATH))
    for name, (restype, argtypes) in PROTOTYPES.items():
        f = getattr(L, name)
        f.restype, f.argtypes = restype, argtypes
    _lib = L
    return L


_host_lib = None


def load_host_library():
    """libabneutral_host.so: the C++ host layer's serial forms (host/host_capi.cpp), built beside the HIP library"""
    global _host_lib
    if _host_lib is None:
        if not _build.PEDIGREE_LIB.exists():
            _build.build_host()
        _host_lib = C.CDLL(str(_build.PEDIGREE_LIB))
    return _host_lib


_POINTERS = {np.dtype(t): C.POINTER(c) for t, c in (
    (np.float64, C.c_double), (np.int32, C.c_int32), (np.int64, C.c_int64), (np.uint8, C.c_uint8),
    (np.uint32, C.c_uint32), (np.uint64, C.c_uint64))}
_POINTERS[FIT_INFO_DTYPE] = C.c_void_p


def _ptr(a):
    """the pointer of an array's own element type (an abn_fit_info record array: void*); None stays None"""
    return None if a is None else a.ctypes.data_as(_POINTERS[a.dtype])


def _dev(p):
    """a raw device address as void*; 0 = not wanted"""
    return C.c_void_p(p or None)


def _arr(a, dtype, shape=None):
    a = np.ascontiguousarray(a, dtype=dtype)
    return a if shape is None else a.reshape(shape)


def _f64(a, shape=None):
    return _arr(a, np.float64, shape)


def _opt(options):
    return C.byref(options) if options else None


def _window_ranges(begin, end):
    b, e = _arr(begin, np.int64), _arr(end, np.int64)
    if b.ndim != 1 or b.shape != e.shape:
        raise ValueError("begin and end are 1-d arrays of one length")
    return b, e


def _pair_outputs(n_samples, lead=()):
    """zeroed (diff u64, both u64, dvalue f64), each (*lead, pairs)"""
    shape = (*lead, n_samples * (n_samples - 1) // 2)
    return np.zeros(shape, dtype=np.uint64), np.zeros(shape, dtype=np.uint64), np.zeros(shape)


def _pair_tables(n_samples, lead=()):
    """the zeroed transition tables u64 (*lead, pairs, 3, 3)"""
    return np.zeros((*lead, n_samples * (n_samples - 1) // 2, 3, 3), dtype=np.uint64)


def _sites_handles(sites_list):
    """(n, abn_sites*[n]) of a list of Sites"""
    sites_list = list(sites_list)
    return len(sites_list), (C.c_void_p * max(len(sites_list), 1))(*(s._h for s in sites_list))


def _sort_info(info):
    return {"sites": int(info[0]), "descents": int(info[1]), "equal": int(info[2]), "passes": int(info[3])}


class _Handle:
    """A handle of the library (`_h`, made by the subclass through `_L`) and its end: `_DESTROY` names the entry point that
    frees it, called once — by close() or when the object is collected.  `_PREFIX` is the C prefix of the entry points
    that `_entry` looks up for the classes that share methods."""

    _DESTROY = ""
    _PREFIX = ""
    _h = None

    @classmethod
    def _new(cls, ctx: "Context"):
        """an instance of ctx, its handle still to be made (the alternative constructors)"""
        self = cls.__new__(cls)
        self.ctx, self._L = ctx, ctx._L
        return self

    def _entry(self, name):
        return getattr(self._L, f"{self._PREFIX}_{name}")

    def _check(self, rc):
        self.ctx._check(rc)

    def _ms(self, entry, n, *index):
        """the n kernel ms an entry point (handle, *index, double*) reports"""
        ms = np.zeros(n)
        self._check(entry(self._h, *index, _ptr(ms)))
        return ms

    def close(self):
        if self._h:
            getattr(self._L, self._DESTROY)(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
