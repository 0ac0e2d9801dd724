"""alphabeta_rs_amd — MI355X-native ABneutral hot path (ctypes binding of the C-ABI in include/abneutral.h).

The compute path is libabneutral_hip.so (hand-written HIP for gfx950).  There is no CPU fallback: if the
library is missing or no HIP device is usable, calls raise.  PyTorch is used by callers only for
`torch.distributed` (RCCL) and stream plumbing, never for the arithmetic.

Python-level names mirror the reference crate: `Pedigree`, `Model`, `ab_neutral.run`, `boot_model.run`
(see alphabeta_rs_amd/api.py); this module is the thin FFI layer.
"""
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

# every symbol include/abneutral.h declares (checked by tests/test_abi.py)
EXPORTED_SYMBOLS = [
    "abn_default_options", "abn_device_count", "abn_init", "abn_shutdown", "abn_device_info", "abn_last_error",
    "abn_status_string", "abn_version", "abn_cost_batch", "abn_fit_batch", "abn_gen_start_simplices",
    "abn_gen_boot_simplices", "abn_gen_boot_indices", "abn_ab_neutral_run", "abn_boot_model_run",
    "abn_analyze", "abn_select_best", "abn_bootstrap_rows", "abn_pairwise_divergence", "abn_plan_create", "abn_plan_destroy", "abn_plan_set_windows", "abn_plan_run",
    "abn_plan_run_phase", "abn_plan_sync", "abn_plan_tail_handed", "abn_plan_set_early_bootstraps", "abn_plan_early_bootstraps", "abn_plan_kernel_ms", "abn_plan_raw_device_ptr",
    "abn_plan_bind_raw", "abn_plan_download", "abn_plan_counters", "abn_plan_device_bytes",
    "abn_plan_set_window_ids", "abn_plan_failed_windows",
    "abn_multi_create", "abn_multi_destroy", "abn_multi_last_error", "abn_multi_set_windows", "abn_multi_run",
    "abn_multi_sync", "abn_multi_shard", "abn_multi_raw_device_ptr", "abn_multi_download", "abn_multi_counters",
    "abn_multi_rccl_available", "abn_reduction_tree", "abn_pairwise_divergence_dev", "abn_multi_set_window_ids",
    "abn_pairwise_divergence_windows", "abn_pairwise_divergence_windows_dev",
    "abn_multi_plan_shard", "abn_plan_last_kernels", "abn_multi_kernel_ms",
    "abn_packed_row_stride", "abn_pack_codes", "abn_unpack_codes", "abn_pairwise_divergence_packed",
    "abn_pairwise_divergence_packed_dev",
    "abn_pairwise_divergence_windows_packed", "abn_pairwise_divergence_windows_packed_dev",
    "abn_analyze_batch", "abn_analyze_batch_dev", "abn_plan_analyze", "abn_multi_analyze",
    "abn_windows_create", "abn_windows_destroy", "abn_windows_info", "abn_windows_stats", "abn_windows_layout",
    "abn_windows_packed", "abn_windows_packed_device_ptr", "abn_windows_pairwise",
    "abn_sites_parse", "abn_sites_destroy", "abn_sites_info", "abn_sites_fetch", "abn_sites_deferred",
    "abn_genes_create", "abn_genes_destroy", "abn_genes_choose", "abn_genes_choose_dev", "abn_windows_create_sites",
    "abn_sites_parse_dev", "abn_sites_flagged", "abn_sites_insert", "abn_windows_create_parsed", "abn_windows_merge_ms",
    "abn_plan_set_stream_sweep", "abn_plan_stream_sweep", "abn_multi_set_stream_sweep", "abn_fit_batch_sweep",
    "abn_codes_create_parsed", "abn_codes_destroy", "abn_codes_info", "abn_codes_stats", "abn_codes_packed",
    "abn_codes_packed_device_ptr", "abn_codes_pairwise", "abn_codes_kernel_ms",
    "abn_sites_common", "abn_sites_common_dev", "abn_windows_create_aligned", "abn_codes_create_aligned",
    "abn_windows_common", "abn_codes_common",
    "abn_sites_union", "abn_sites_union_dev", "abn_windows_create_union", "abn_codes_create_union",
    "abn_windows_union", "abn_codes_union",
    "abn_tiles_create", "abn_tiles_destroy", "abn_tiles_info", "abn_tiles_runs", "abn_tiles_set_intervals",
    "abn_tiles_set_fixed", "abn_tiles_intervals", "abn_tiles_layout", "abn_tiles_stats", "abn_tiles_pairwise",
    "abn_tiles_kernel_ms",
    "abn_tiles_set_pools", "abn_tiles_pool_segments", "abn_tiles_pool_columns", "abn_tiles_pool_kernel_ms",
    "abn_sites_context", "abn_sites_insert_ctx", "abn_sites_split", "abn_sites_split_ms",
    "abn_sites_sort", "abn_sites_sort_order", "abn_sites_sort_info", "abn_sites_sort_keys", "abn_sites_sort_keys_dev",
    "abn_pairwise_transitions_packed", "abn_pairwise_transitions_packed_dev",
    "abn_pairwise_transitions_windows_packed", "abn_pairwise_transitions_windows_packed_dev",
    "abn_codes_transitions", "abn_tiles_transitions",
    "abn_block_counts", "abn_block_counts_host", "abn_block_resample", "abn_block_resample_dev",
    "abn_block_resample_host", "abn_tiles_block_bootstrap", "abn_tiles_block_groups", "abn_tiles_block_ms",
]


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


CONTEXTS = ("CG", "CHG", "CHH")  # a site's context code indexes it; code 3: a row without a context


def _context_mask(contexts) -> int:
    """("CG", "CHH") or "CG,CHH" or the mask itself -> abn_sites_params.contexts (1 CG, 2 CHG, 4 CHH)"""
    if isinstance(contexts, (int, np.integer)):
        return int(contexts)
    names = contexts.split(",") if isinstance(contexts, str) else list(contexts)
    if not names or len(set(names)) != len(names) or any(n not in CONTEXTS for n in names):
        raise ValueError(f"contexts expects distinct names of {CONTEXTS}, not {contexts!r}")
    return sum(1 << CONTEXTS.index(n) for n in names)


class AbnError(RuntimeError):
    def __init__(self, status: int, detail: str = ""):
        self.status = status
        super().__init__(f"{STATUS_NAMES.get(status, status)}: {detail}")


_lib = None


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
    dp, u32p, vp = C.POINTER(C.c_double), C.POINTER(C.c_uint32), C.c_void_p
    op = C.POINTER(Options)
    L.abn_default_options.argtypes = [op]
    L.abn_default_options.restype = None
    L.abn_device_count.argtypes = [C.POINTER(C.c_int)]
    L.abn_init.argtypes = [C.c_int, vp, C.POINTER(vp)]
    L.abn_shutdown.argtypes = [vp]
    L.abn_device_info.argtypes = [vp, C.POINTER(C.c_int32)]
    L.abn_last_error.argtypes = [vp]
    L.abn_last_error.restype = C.c_char_p
    L.abn_status_string.argtypes = [C.c_int]
    L.abn_status_string.restype = C.c_char_p
    L.abn_cost_batch.argtypes = [vp, op, dp, C.c_int32, C.c_double, C.c_double, C.c_double, dp, C.c_int64, dp, dp,
                                 u32p, u32p, C.c_int64, dp, dp, dp]
    L.abn_fit_batch.argtypes = [vp, op, dp, C.c_int32, C.c_double, C.c_double, C.c_double, dp, C.c_int64, dp,
                                C.c_int32, dp, vp]
    L.abn_fit_batch_sweep.argtypes = [vp, op, dp, C.c_int32, C.c_double, C.c_double, C.c_double, dp, C.c_int64, dp,
                                      C.c_int32, dp, vp, C.POINTER(C.c_int64)]
    L.abn_gen_start_simplices.argtypes = [C.c_uint64, C.c_uint32, C.c_int32, C.c_double, dp]
    L.abn_gen_boot_simplices.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32, C.c_int64, dp, dp]
    L.abn_gen_boot_indices.argtypes = [vp, C.c_uint64, C.c_uint32, C.c_uint32, C.c_int64, C.c_int32, u32p]
    L.abn_ab_neutral_run.argtypes = [vp, op, dp, C.c_int32, C.c_double, C.c_double, C.c_double, C.c_int32, dp, dp,
                                     dp, dp, vp, dp]
    L.abn_boot_model_run.argtypes = [vp, op, dp, C.c_int32, dp, dp, dp, C.c_double, C.c_double, C.c_double,
                                     C.c_int32, dp, vp]
    L.abn_analyze.argtypes = [dp, C.c_int64, dp]
    L.abn_analyze_batch.argtypes = [vp, dp, C.c_int32, C.c_int64, dp, C.POINTER(C.c_int32)]
    L.abn_analyze_batch_dev.argtypes = [vp, vp, C.c_int32, C.c_int64, vp, vp, dp]
    L.abn_plan_analyze.argtypes = [vp, dp, C.POINTER(C.c_int32)]
    L.abn_multi_analyze.argtypes = [vp, dp, C.POINTER(C.c_int32)]
    L.abn_select_best.argtypes = [vp, dp, C.c_int32, C.c_double, dp, C.c_int32, C.POINTER(C.c_int32), dp, dp, dp, dp]
    L.abn_bootstrap_rows.argtypes = [vp, dp, C.c_int64, dp]
    L.abn_pairwise_divergence.argtypes = [vp, C.POINTER(C.c_uint8), C.c_int32, C.c_int64, C.POINTER(C.c_uint64),
                                          C.POINTER(C.c_uint64), dp]
    L.abn_pairwise_divergence_dev.argtypes = [vp, vp, C.c_int32, C.c_int64, vp, vp, vp, dp]
    i64p = C.POINTER(C.c_int64)
    L.abn_pairwise_divergence_windows.argtypes = [vp, C.POINTER(C.c_uint8), C.c_int32, C.c_int64, i64p, i64p, C.c_int32,
                                                  C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), dp]
    L.abn_pairwise_divergence_windows_dev.argtypes = [vp, vp, C.c_int32, C.c_int64, i64p, i64p, C.c_int32, vp, vp, vp, dp]
    u8p = C.POINTER(C.c_uint8)
    L.abn_packed_row_stride.argtypes = [C.c_int64]
    L.abn_packed_row_stride.restype = C.c_int64
    L.abn_pack_codes.argtypes = [u8p, C.c_int32, C.c_int64, C.c_int64, u8p, C.c_int64]
    L.abn_unpack_codes.argtypes = [u8p, C.c_int32, C.c_int64, C.c_int64, u8p, C.c_int64]
    L.abn_pairwise_divergence_packed.argtypes = [vp, u8p, C.c_int32, C.c_int64, C.c_int64, C.POINTER(C.c_uint64),
                                                 C.POINTER(C.c_uint64), dp]
    L.abn_pairwise_divergence_packed_dev.argtypes = [vp, vp, C.c_int32, C.c_int64, C.c_int64, vp, vp, vp, dp]
    L.abn_pairwise_divergence_windows_packed.argtypes = [vp, u8p, C.c_int32, C.c_int64, C.c_int64, i64p, i64p, C.c_int32,
                                                         C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), dp]
    L.abn_pairwise_divergence_windows_packed_dev.argtypes = [vp, vp, C.c_int32, C.c_int64, C.c_int64, i64p, i64p,
                                                             C.c_int32, vp, vp, vp, dp]
    u64p = C.POINTER(C.c_uint64)
    L.abn_pairwise_transitions_packed.argtypes = [vp, u8p, C.c_int32, C.c_int64, C.c_int64, u64p]
    L.abn_pairwise_transitions_packed_dev.argtypes = [vp, vp, C.c_int32, C.c_int64, C.c_int64, vp, dp]
    L.abn_pairwise_transitions_windows_packed.argtypes = [vp, u8p, C.c_int32, C.c_int64, C.c_int64, i64p, i64p,
                                                          C.c_int32, u64p]
    L.abn_pairwise_transitions_windows_packed_dev.argtypes = [vp, vp, C.c_int32, C.c_int64, C.c_int64, i64p, i64p,
                                                              C.c_int32, vp, dp]
    L.abn_codes_transitions.argtypes = [vp, u64p]
    L.abn_tiles_transitions.argtypes = [vp, u64p]
    L.abn_windows_create.argtypes = [vp, C.POINTER(WindowsParams), C.c_int32, i64p, u32p, u32p, u32p, u8p, u8p, dp,
                                     C.POINTER(vp)]
    L.abn_windows_destroy.argtypes = [vp]
    L.abn_windows_info.argtypes = [vp, C.POINTER(C.c_int32), i64p, i64p]
    L.abn_windows_stats.argtypes = [vp, i64p, dp, dp, i64p]
    L.abn_windows_layout.argtypes = [vp, i64p, i64p, C.POINTER(C.c_int32)]
    L.abn_windows_packed.argtypes = [vp, u8p]
    L.abn_windows_packed_device_ptr.argtypes = [vp, C.POINTER(vp)]
    L.abn_windows_pairwise.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), dp]
    L.abn_sites_parse.argtypes = [vp, C.c_char_p, C.c_int64, C.POINTER(SitesParams), C.POINTER(vp)]
    L.abn_sites_destroy.argtypes = [vp]
    L.abn_sites_info.argtypes = [vp, i64p, i64p, i64p, dp]
    L.abn_sites_fetch.argtypes = [vp, i64p, C.POINTER(C.c_int32), u32p, u32p, u8p, dp, u8p, u8p, dp]
    L.abn_sites_deferred.argtypes = [vp, i64p, i64p, i64p]
    L.abn_sites_parse_dev.argtypes = [vp, C.c_char_p, C.c_int64, C.POINTER(SitesParams), C.POINTER(vp)]
    L.abn_sites_flagged.argtypes = [vp, i64p, i64p]
    L.abn_sites_insert.argtypes = [vp, C.c_int64, i64p, C.POINTER(C.c_int32), u32p, u32p, u8p, dp, u8p, dp]
    L.abn_sites_insert_ctx.argtypes = [*L.abn_sites_insert.argtypes, u8p]
    L.abn_sites_context.argtypes = [vp, C.POINTER(C.c_int32), u8p]
    L.abn_sites_split.argtypes = [vp, C.POINTER(vp)]
    L.abn_sites_split_ms.argtypes = [vp, dp]
    L.abn_sites_sort.argtypes = [vp, C.POINTER(vp)]
    L.abn_sites_sort_order.argtypes = [vp, i64p, i64p]
    L.abn_sites_sort_info.argtypes = [vp, i64p, dp]
    L.abn_sites_sort_keys.argtypes = [vp, C.c_int64, C.POINTER(C.c_int32), u32p, u32p, u8p, i64p, i64p]
    L.abn_sites_sort_keys_dev.argtypes = [vp, C.c_int64, vp, vp, vp, vp, vp, i64p, dp]
    L.abn_windows_create_parsed.argtypes = [vp, C.POINTER(WindowsParams), vp, C.POINTER(GeneRule), C.c_double, C.c_int32,
                                            C.POINTER(vp), C.POINTER(vp)]
    L.abn_windows_merge_ms.argtypes = [vp, dp]
    L.abn_codes_create_parsed.argtypes = [vp, C.c_double, C.c_int32, C.POINTER(vp), C.POINTER(vp)]
    L.abn_codes_destroy.argtypes = [vp]
    L.abn_codes_info.argtypes = [vp, C.POINTER(C.c_int32), i64p, i64p, C.POINTER(C.c_int32)]
    L.abn_codes_stats.argtypes = [vp, i64p, dp, i64p]
    L.abn_codes_packed.argtypes = [vp, u8p]
    L.abn_codes_packed_device_ptr.argtypes = [vp, C.POINTER(vp)]
    L.abn_codes_pairwise.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), dp]
    L.abn_codes_kernel_ms.argtypes = [vp, dp]
    L.abn_sites_common.argtypes = [vp, C.c_int32, i64p, C.POINTER(C.c_int32), u32p, u32p, u8p, u8p, i64p]
    L.abn_sites_common_dev.argtypes = [vp, C.c_int32, i64p, vp, vp, vp, vp, vp, i64p]
    L.abn_windows_create_aligned.argtypes = L.abn_windows_create_parsed.argtypes
    L.abn_codes_create_aligned.argtypes = L.abn_codes_create_parsed.argtypes
    L.abn_windows_common.argtypes = [vp, i64p, i64p, dp]
    L.abn_codes_common.argtypes = [vp, i64p, i64p, dp]
    L.abn_sites_union.argtypes = [vp, C.c_int32, i64p, C.POINTER(C.c_int32), u32p, u32p, u8p, u32p, i64p]
    L.abn_sites_union_dev.argtypes = [vp, C.c_int32, i64p, vp, vp, vp, vp, vp, i64p]
    L.abn_windows_create_union.argtypes = L.abn_windows_create_parsed.argtypes
    L.abn_codes_create_union.argtypes = L.abn_codes_create_parsed.argtypes
    L.abn_windows_union.argtypes = [vp, i64p, i64p, dp]
    L.abn_codes_union.argtypes = [vp, i64p, i64p, dp]
    i32p = C.POINTER(C.c_int32)
    L.abn_tiles_create.argtypes = [vp, C.c_double, C.c_int32, C.c_int32, C.POINTER(vp), C.POINTER(vp)]
    L.abn_tiles_destroy.argtypes = [vp]
    L.abn_tiles_info.argtypes = [vp, i32p, i64p, i64p, i32p, i64p]
    L.abn_tiles_runs.argtypes = [vp, i32p, i64p, i64p, u32p]
    L.abn_tiles_set_intervals.argtypes = [vp, C.c_int64, i32p, i64p, i64p]
    L.abn_tiles_set_fixed.argtypes = [vp, C.c_int64, C.c_int64]
    L.abn_tiles_intervals.argtypes = [vp, i32p, i64p, i64p]
    L.abn_tiles_layout.argtypes = [vp, i64p, i64p]
    L.abn_tiles_stats.argtypes = [vp, i64p, dp, i64p]
    L.abn_tiles_pairwise.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), dp]
    L.abn_tiles_kernel_ms.argtypes = [vp, dp]
    L.abn_tiles_set_pools.argtypes = [vp, C.c_int64, i32p, i64p, i64p, i32p, C.c_int64]
    L.abn_tiles_pool_segments.argtypes = [vp, i64p, i32p, i32p, i64p, i64p, i64p, i64p]
    L.abn_tiles_pool_columns.argtypes = [vp, i64p]
    L.abn_tiles_pool_kernel_ms.argtypes = [vp, dp]
    groups = [C.c_int32, i64p, i64p]
    L.abn_block_counts.argtypes = [vp, C.c_uint64, C.c_int32, u32p, i64p, i64p, C.c_int64, C.c_int64, u8p]
    L.abn_block_counts_host.argtypes = [*L.abn_block_counts.argtypes[1:], C.c_char_p, C.c_int32]
    L.abn_block_resample.argtypes = [vp, *groups, C.c_int64, u8p, C.c_int64, C.c_int64, C.c_int32, u64p, u64p, dp, i64p,
                                     u64p, u64p, dp, dp, i64p]
    L.abn_block_resample_host.argtypes = [*L.abn_block_resample.argtypes[1:], C.c_char_p, C.c_int32]
    L.abn_block_resample_dev.argtypes = [vp, *groups, C.c_int64, vp, C.c_int64, C.c_int64, C.c_int32, vp, vp, vp, vp,
                                         vp, vp, vp, vp, vp, dp]
    L.abn_tiles_block_bootstrap.argtypes = [vp, C.c_uint64, C.c_int64, u64p, u64p, dp, dp, i64p]
    L.abn_tiles_block_ms.argtypes = [vp, dp]
    L.abn_tiles_block_groups.argtypes = [vp, i64p, i64p, i64p, i64p]
    L.abn_genes_create.argtypes = [vp, C.c_int32, i32p, i32p, i64p, u32p, u32p, u8p, C.POINTER(vp)]
    L.abn_genes_destroy.argtypes = [vp]
    L.abn_genes_choose.argtypes = [vp, C.POINTER(GeneRule), C.c_int32, i64p, i32p, u32p, u32p, u8p, u32p, u32p, u8p, dp]
    L.abn_genes_choose_dev.argtypes = [vp, C.POINTER(GeneRule), C.c_int32, i64p, vp, vp, vp, vp, vp, vp, vp, dp]
    L.abn_windows_create_sites.argtypes = [vp, C.POINTER(WindowsParams), vp, C.POINTER(GeneRule), C.c_int32, i64p, i32p,
                                           u32p, u32p, u8p, u8p, dp, C.POINTER(vp)]
    L.abn_plan_create.argtypes = [vp, op, dp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_uint32, C.c_uint32,
                                  C.POINTER(vp)]
    L.abn_plan_destroy.argtypes = [vp]
    L.abn_plan_set_windows.argtypes = [vp, dp, dp, dp, dp]
    L.abn_plan_run.argtypes = [vp]
    L.abn_plan_run_phase.argtypes = [vp, C.c_int32]
    L.abn_plan_sync.argtypes = [vp]
    L.abn_plan_tail_handed.argtypes = [vp, C.POINTER(C.c_int64)]
    L.abn_plan_set_early_bootstraps.argtypes = [vp, C.c_int32]
    L.abn_plan_set_stream_sweep.argtypes = [vp, C.c_int32]
    L.abn_plan_stream_sweep.argtypes = [vp, C.POINTER(C.c_int64)]
    L.abn_multi_set_stream_sweep.argtypes = [vp, C.c_int32]
    L.abn_plan_early_bootstraps.argtypes = [vp, C.POINTER(C.c_int32)]
    L.abn_plan_kernel_ms.argtypes = [vp, dp]
    L.abn_plan_raw_device_ptr.argtypes = [vp, C.POINTER(vp)]
    L.abn_plan_bind_raw.argtypes = [vp, vp]
    L.abn_plan_download.argtypes = [vp, dp, dp, dp, dp, vp, vp, C.POINTER(C.c_int32)]
    L.abn_plan_counters.argtypes = [vp, C.POINTER(C.c_int64)]
    L.abn_plan_device_bytes.argtypes = [vp, C.POINTER(C.c_int64)]
    L.abn_plan_set_window_ids.argtypes = [vp, u32p]
    L.abn_plan_failed_windows.argtypes = [vp, C.POINTER(C.c_int32)]
    L.abn_plan_last_kernels.argtypes = [vp, C.POINTER(C.c_int32)]
    i32p = C.POINTER(C.c_int32)
    L.abn_multi_create.argtypes = [i32p, C.c_int32, op, dp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(vp)]
    L.abn_multi_destroy.argtypes = [vp]
    L.abn_multi_last_error.argtypes = [vp]
    L.abn_multi_last_error.restype = C.c_char_p
    L.abn_multi_set_windows.argtypes = [vp, dp, dp, dp, dp]
    L.abn_multi_set_window_ids.argtypes = [vp, u32p]
    L.abn_multi_run.argtypes = [vp]
    L.abn_multi_sync.argtypes = [vp]
    L.abn_multi_shard.argtypes = [vp, C.c_int32, i32p]
    L.abn_multi_plan_shard.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int32, i32p]
    L.abn_multi_raw_device_ptr.argtypes = [vp, C.c_int32, C.POINTER(vp)]
    L.abn_multi_kernel_ms.argtypes = [vp, C.c_int32, dp]
    L.abn_multi_download.argtypes = [vp, dp, dp, dp, dp, vp, vp, i32p]
    L.abn_multi_counters.argtypes = [vp, C.POINTER(C.c_int64)]
    L.abn_multi_rccl_available.argtypes = [C.POINTER(C.c_int)]
    L.abn_reduction_tree.argtypes = [op, dp, C.c_int32, i32p]
    _lib = L
    return L


def _dp(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))


def _u32p(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_uint32))


def _f64(a, shape=None):
    a = np.ascontiguousarray(a, dtype=np.float64)
    return a if shape is None else a.reshape(shape)


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
    rc = load_library().abn_gen_start_simplices(seed, window, n_starts, max_divergence, _dp(out))
    if rc:
        raise AbnError(rc)
    return out


def gen_boot_simplices(seed: int, window: int, b0: int, nb: int, params) -> np.ndarray:
    p = _f64(params, (4,))
    out = np.empty((nb, 5, 4))
    rc = load_library().abn_gen_boot_simplices(seed, window, b0, nb, _dp(p), _dp(out))
    if rc:
        raise AbnError(rc)
    return out


def packed_row_stride(n_sites: int) -> int:
    """Bytes per row of 2-bit packed codes for n_sites sites: ceil(n_sites / 256) * 64 (host arithmetic)."""
    return int(load_library().abn_packed_row_stride(int(n_sites)))


def pack_codes(codes, row_stride: int | None = None) -> np.ndarray:
    """(n_samples, n_sites) u8 codes (status | 0x80 if filtered) -> (n_samples, row_stride) u8 rows of 2-bit fields, the
    input of Context.pairwise_divergence_packed (format: include/abneutral.h).  row_stride: a multiple of 64, default
    packed_row_stride(n_sites).  Host arithmetic; a byte that is no code raises AbnError."""
    codes = np.ascontiguousarray(codes, dtype=np.uint8)
    n, L = codes.shape
    stride = packed_row_stride(L) if row_stride is None else int(row_stride)
    packed = np.empty((n, max(stride, 0)), dtype=np.uint8)
    u8p = C.POINTER(C.c_uint8)
    rc = load_library().abn_pack_codes(codes.ctypes.data_as(u8p), n, L, L, packed.ctypes.data_as(u8p), stride)
    if rc != 0:
        raise AbnError(rc, "pack_codes: a byte that is not 0, 1, 2 or 0x80 | status, or a bad row stride")
    return packed


def unpack_codes(packed, n_sites: int) -> np.ndarray:
    """(n_samples, row_stride) packed rows -> (n_samples, n_sites) u8 codes; filtered sites come back as 0x80."""
    packed = np.ascontiguousarray(packed, dtype=np.uint8)
    n, stride = packed.shape
    codes = np.empty((n, int(n_sites)), dtype=np.uint8)
    u8p = C.POINTER(C.c_uint8)
    rc = load_library().abn_unpack_codes(packed.ctypes.data_as(u8p), n, int(n_sites), stride, codes.ctypes.data_as(u8p),
                                         int(n_sites))
    if rc != 0:
        raise AbnError(rc, "unpack_codes: bad row stride")
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
    rc = load_library().abn_analyze(_dp(raw), raw.shape[0], _dp(out))
    if rc:
        raise AbnError(rc)
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
    rc = ctx._L.abn_analyze_batch(ctx._h, _dp(raw), W, B, _dp(out), fb.ctypes.data_as(C.POINTER(C.c_int32)))
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
            idx = np.ascontiguousarray(idx, dtype=np.uint32).reshape(-1, n)
            nb = idx.shape[0]
            pred, resid = _f64(pred, (n,)), _f64(resid, (n,))
            if cand_to_boot is not None:
                cand_to_boot = np.ascontiguousarray(cand_to_boot, dtype=np.uint32).reshape(m)
        self._check(self._L.abn_cost_batch(self._h, C.byref(options) if options else None, _dp(ped), n, p_uu0, eqp,
                                           eqp_weight, _dp(cand), m, _dp(pred), _dp(resid), _u32p(idx),
                                           _u32p(cand_to_boot), nb, _dp(cost), _dp(dt), _dp(puu)))
        out = [cost]
        if want_dt:
            out.append(dt)
        if want_puu:
            out.append(puu)
        return out[0] if len(out) == 1 else tuple(out)

    # ---- Nelder-Mead fits from explicit start simplices
    def fit_batch(self, pedigree, p_uu0, eqp, eqp_weight, simplex0, max_iters, *, dobs_rows=None,
                  options: Options | None = None):
        ped = _f64(pedigree).reshape(-1, 4)
        s0 = _f64(simplex0).reshape(-1, 20)
        n, f = ped.shape[0], s0.shape[0]
        d = None if dobs_rows is None else _f64(dobs_rows, (f, n))
        best = np.empty((f, 4))
        info = np.zeros(f, dtype=FIT_INFO_DTYPE)
        self._check(self._L.abn_fit_batch(self._h, C.byref(options) if options else None, _dp(ped), n, p_uu0, eqp,
                                          eqp_weight, _dp(s0), f, _dp(d), max_iters, _dp(best), info.ctypes.data))
        return best, info

    def fit_batch_sweep(self, pedigree, p_uu0, eqp, eqp_weight, simplex0, max_iters, *, dobs_rows=None,
                        options: Options | None = None):
        """fit_batch on the sweep kernel (one pass over the rows per iteration): (best, info, passes over the rows).
        Refused (ABN_ERR_INVALID_ARG) when the pedigree and the options do not route to that kernel."""
        ped = _f64(pedigree).reshape(-1, 4)
        s0 = _f64(simplex0).reshape(-1, 20)
        n, f = ped.shape[0], s0.shape[0]
        d = None if dobs_rows is None else _f64(dobs_rows, (f, n))
        best = np.empty((f, 4))
        info = np.zeros(f, dtype=FIT_INFO_DTYPE)
        passes = C.c_int64(0)
        self._check(self._L.abn_fit_batch_sweep(self._h, C.byref(options) if options else None, _dp(ped), n, p_uu0, eqp,
                                                eqp_weight, _dp(s0), f, _dp(d), max_iters, _dp(best), info.ctypes.data,
                                                C.byref(passes)))
        return best, info, int(passes.value)

    def gen_boot_indices(self, seed, window, b0, nb, n_rows) -> np.ndarray:
        idx = np.empty((nb, n_rows), dtype=np.uint32)
        self._check(self._L.abn_gen_boot_indices(self._h, seed, window, b0, nb, n_rows, _u32p(idx)))
        return idx

    # ---- (2) ab_neutral::run
    def ab_neutral_run(self, pedigree, p0uu, eqp, eqp_weight, n_starts, *, options: Options | None = None):
        ped = _f64(pedigree).reshape(-1, 4)
        n = ped.shape[0]
        model, pred, resid = np.empty(4), np.empty(n), np.empty(n)
        allm = np.empty((n_starts, 4))
        info = np.zeros(n_starts, dtype=FIT_INFO_DTYPE)
        lse = np.empty(n_starts)
        self._check(self._L.abn_ab_neutral_run(self._h, C.byref(options) if options else None, _dp(ped), n, p0uu, eqp,
                                               eqp_weight, n_starts, _dp(model), _dp(pred), _dp(resid), _dp(allm),
                                               info.ctypes.data, _dp(lse)))
        return model, pred, resid, {"models": allm, "info": info, "lse": lse}

    def select_best(self, pedigree, p0uu, models):
        """src/ab_neutral.rs:83-135: (index, model, pred, resid, lse)"""
        ped = _f64(pedigree).reshape(-1, 4)
        m = _f64(models).reshape(-1, 4)
        n = ped.shape[0]
        k = C.c_int32(-1)
        model, pred, resid, lse = np.empty(4), np.empty(n), np.empty(n), np.empty(m.shape[0])
        self._check(self._L.abn_select_best(self._h, _dp(ped), n, p0uu, _dp(m), m.shape[0], C.byref(k), _dp(model),
                                            _dp(pred), _dp(resid), _dp(lse)))
        return k.value, model, pred, resid, lse

    def bootstrap_rows(self, best):
        """src/boot_model.rs:86-91"""
        b = _f64(best).reshape(-1, 4)
        raw = np.empty((b.shape[0], 7))
        self._check(self._L.abn_bootstrap_rows(self._h, _dp(b), b.shape[0], _dp(raw)))
        return raw

    def pairwise_divergence(self, codes):
        """DMatrix::from (src/pedigree.rs:210-261).  codes: (n_samples, n_sites) u8 = status | 0x80 if filtered.
        Returns (diff u64, both u64, dvalue f64), one entry per pair i < j in nested-loop order."""
        codes = np.ascontiguousarray(codes, dtype=np.uint8)
        n, L = codes.shape
        npairs = n * (n - 1) // 2
        diff, both = np.zeros(npairs, dtype=np.uint64), np.zeros(npairs, dtype=np.uint64)
        dval = np.zeros(npairs)
        self._check(self._L.abn_pairwise_divergence(self._h, codes.ctypes.data_as(C.POINTER(C.c_uint8)), n, L,
                                                    diff.ctypes.data_as(C.POINTER(C.c_uint64)),
                                                    both.ctypes.data_as(C.POINTER(C.c_uint64)), _dp(dval)))
        return diff, both, dval

    def pairwise_divergence_dev(self, codes_ptr: int, n_samples: int, n_sites: int, diff_ptr: int = 0,
                                both_ptr: int = 0, dvalue_ptr: int = 0) -> float:
        """The same on device-resident buffers (raw device pointers, e.g. torch tensors' data_ptr()): u8 codes
        [n x L] in, u64 diff / both and f64 dvalue [pairs] out (0 = not wanted).  Returns the kernels' HIP-event ms."""
        ms = C.c_double(0.0)
        self._check(self._L.abn_pairwise_divergence_dev(self._h, C.c_void_p(codes_ptr), n_samples, n_sites,
                                                        C.c_void_p(diff_ptr or None), C.c_void_p(both_ptr or None),
                                                        C.c_void_p(dvalue_ptr or None), C.byref(ms)))
        return ms.value

    def pairwise_divergence_packed(self, packed, n_sites: int):
        """pairwise_divergence on 2-bit packed codes (pack_codes): packed (n_samples, row_stride) u8, n_sites sites per
        sample.  The same (diff, both, dvalue), bit for bit."""
        packed = np.ascontiguousarray(packed, dtype=np.uint8)
        n, stride = packed.shape
        npairs = n * (n - 1) // 2
        diff, both = np.zeros(npairs, dtype=np.uint64), np.zeros(npairs, dtype=np.uint64)
        dval = np.zeros(npairs)
        self._check(self._L.abn_pairwise_divergence_packed(self._h, packed.ctypes.data_as(C.POINTER(C.c_uint8)), n,
                                                           int(n_sites), stride,
                                                           diff.ctypes.data_as(C.POINTER(C.c_uint64)),
                                                           both.ctypes.data_as(C.POINTER(C.c_uint64)), _dp(dval)))
        return diff, both, dval

    def pairwise_divergence_packed_dev(self, packed_ptr: int, n_samples: int, n_sites: int, row_stride: int,
                                       diff_ptr: int = 0, both_ptr: int = 0, dvalue_ptr: int = 0) -> float:
        """The same on device-resident buffers: packed rows [n x row_stride] (16-byte aligned) in, u64 diff / both and
        f64 dvalue [pairs] out (0 = not wanted).  Returns the kernels' HIP-event ms."""
        ms = C.c_double(0.0)
        self._check(self._L.abn_pairwise_divergence_packed_dev(self._h, C.c_void_p(packed_ptr), n_samples, n_sites,
                                                               row_stride, C.c_void_p(diff_ptr or None),
                                                               C.c_void_p(both_ptr or None),
                                                               C.c_void_p(dvalue_ptr or None), C.byref(ms)))
        return ms.value

    def pairwise_divergence_windows(self, codes, begin, end):
        """pairwise_divergence of the column ranges [begin[w], end[w]) of one (n_samples, row_stride) code matrix in one
        batched call (the window loop of src/cli/metaprofile.rs:50-72).  Returns (diff, both, dvalue), each of shape
        (n_windows, pairs), bit-identical to pairwise_divergence(codes[:, b:e]) per window."""
        codes = np.ascontiguousarray(codes, dtype=np.uint8)
        n, stride = codes.shape
        b, e = np.ascontiguousarray(begin, dtype=np.int64), np.ascontiguousarray(end, dtype=np.int64)
        if b.ndim != 1 or b.shape != e.shape:
            raise ValueError("begin and end are 1-d arrays of one length")
        W, npairs = b.shape[0], n * (n - 1) // 2
        diff, both = np.zeros((W, npairs), dtype=np.uint64), np.zeros((W, npairs), dtype=np.uint64)
        dval = np.zeros((W, npairs))
        i64p = C.POINTER(C.c_int64)
        self._check(self._L.abn_pairwise_divergence_windows(
            self._h, codes.ctypes.data_as(C.POINTER(C.c_uint8)), n, stride, b.ctypes.data_as(i64p),
            e.ctypes.data_as(i64p), W, diff.ctypes.data_as(C.POINTER(C.c_uint64)),
            both.ctypes.data_as(C.POINTER(C.c_uint64)), _dp(dval)))
        return diff, both, dval

    def pairwise_divergence_windows_dev(self, codes_ptr: int, n_samples: int, row_stride: int, begin, end,
                                        diff_ptr: int = 0, both_ptr: int = 0, dvalue_ptr: int = 0) -> float:
        """The same on device-resident buffers: u8 codes [n x row_stride] in, u64 diff / both and f64 dvalue
        [n_windows x pairs] out (0 = not wanted); begin / end are host arrays.  Returns the kernels' HIP-event ms."""
        b, e = np.ascontiguousarray(begin, dtype=np.int64), np.ascontiguousarray(end, dtype=np.int64)
        if b.ndim != 1 or b.shape != e.shape:
            raise ValueError("begin and end are 1-d arrays of one length")
        ms = C.c_double(0.0)
        i64p = C.POINTER(C.c_int64)
        self._check(self._L.abn_pairwise_divergence_windows_dev(
            self._h, C.c_void_p(codes_ptr), n_samples, row_stride, b.ctypes.data_as(i64p), e.ctypes.data_as(i64p),
            b.shape[0], C.c_void_p(diff_ptr or None), C.c_void_p(both_ptr or None), C.c_void_p(dvalue_ptr or None),
            C.byref(ms)))
        return ms.value

    def pairwise_divergence_windows_packed(self, packed, n_sites: int, begin, end):
        """pairwise_divergence_windows on 2-bit packed codes (pack_codes): packed (n_samples, row_stride) u8 with n_sites
        sites per sample; windows [begin[w], end[w]) in sites, at any site.  Returns (diff, both, dvalue), each of shape
        (n_windows, pairs), bit-identical to pairwise_divergence_windows on the unpacked codes."""
        packed = np.ascontiguousarray(packed, dtype=np.uint8)
        n, stride = packed.shape
        b, e = np.ascontiguousarray(begin, dtype=np.int64), np.ascontiguousarray(end, dtype=np.int64)
        if b.ndim != 1 or b.shape != e.shape:
            raise ValueError("begin and end are 1-d arrays of one length")
        W, npairs = b.shape[0], n * (n - 1) // 2
        diff, both = np.zeros((W, npairs), dtype=np.uint64), np.zeros((W, npairs), dtype=np.uint64)
        dval = np.zeros((W, npairs))
        i64p = C.POINTER(C.c_int64)
        self._check(self._L.abn_pairwise_divergence_windows_packed(
            self._h, packed.ctypes.data_as(C.POINTER(C.c_uint8)), n, int(n_sites), stride, b.ctypes.data_as(i64p),
            e.ctypes.data_as(i64p), W, diff.ctypes.data_as(C.POINTER(C.c_uint64)),
            both.ctypes.data_as(C.POINTER(C.c_uint64)), _dp(dval)))
        return diff, both, dval

    def pairwise_divergence_windows_packed_dev(self, packed_ptr: int, n_samples: int, n_sites: int, row_stride: int,
                                               begin, end, diff_ptr: int = 0, both_ptr: int = 0,
                                               dvalue_ptr: int = 0) -> float:
        """The same on device-resident buffers: packed rows [n x row_stride] (16-byte aligned) in, u64 diff / both and
        f64 dvalue [n_windows x pairs] out (0 = not wanted); begin / end are host arrays.  Returns the kernels'
        HIP-event ms."""
        b, e = np.ascontiguousarray(begin, dtype=np.int64), np.ascontiguousarray(end, dtype=np.int64)
        if b.ndim != 1 or b.shape != e.shape:
            raise ValueError("begin and end are 1-d arrays of one length")
        ms = C.c_double(0.0)
        i64p = C.POINTER(C.c_int64)
        self._check(self._L.abn_pairwise_divergence_windows_packed_dev(
            self._h, C.c_void_p(packed_ptr), n_samples, n_sites, row_stride, b.ctypes.data_as(i64p),
            e.ctypes.data_as(i64p), b.shape[0], C.c_void_p(diff_ptr or None), C.c_void_p(both_ptr or None),
            C.c_void_p(dvalue_ptr or None), C.byref(ms)))
        return ms.value

    def pairwise_transitions_packed(self, packed, n_sites: int):
        """The 3 x 3 state transitions of every pair on 2-bit packed codes (pack_codes): uint64 (pairs, 3, 3), entry
        [p, x, y] = the sites both samples of pair p = (a, b), a < b, keep with status x in a and y in b (0 = U, 1 = I,
        2 = M).  Its sum is pairwise_divergence_packed's both, its |x - y|-weighted sum the diff."""
        packed = np.ascontiguousarray(packed, dtype=np.uint8)
        n, stride = packed.shape
        table = np.zeros((n * (n - 1) // 2, 3, 3), dtype=np.uint64)
        self._check(self._L.abn_pairwise_transitions_packed(self._h, packed.ctypes.data_as(C.POINTER(C.c_uint8)), n,
                                                            int(n_sites), stride,
                                                            table.ctypes.data_as(C.POINTER(C.c_uint64))))
        return table

    def pairwise_transitions_packed_dev(self, packed_ptr: int, n_samples: int, n_sites: int, row_stride: int,
                                        table_ptr: int) -> float:
        """The same on device-resident buffers: packed rows [n x row_stride] (16-byte aligned) in, u64 table
        [pairs x 9] out.  Returns the kernels' HIP-event ms."""
        ms = C.c_double(0.0)
        self._check(self._L.abn_pairwise_transitions_packed_dev(self._h, C.c_void_p(packed_ptr), n_samples, n_sites,
                                                                row_stride, C.c_void_p(table_ptr or None), C.byref(ms)))
        return ms.value

    def pairwise_transitions_windows_packed(self, packed, n_sites: int, begin, end):
        """pairwise_transitions_packed of the column ranges [begin[w], end[w]) (in sites, at any site) of one packed
        matrix in one batched call: uint64 (n_windows, pairs, 3, 3); an empty window's table is zero."""
        packed = np.ascontiguousarray(packed, dtype=np.uint8)
        n, stride = packed.shape
        b, e = np.ascontiguousarray(begin, dtype=np.int64), np.ascontiguousarray(end, dtype=np.int64)
        if b.ndim != 1 or b.shape != e.shape:
            raise ValueError("begin and end are 1-d arrays of one length")
        table = np.zeros((b.shape[0], n * (n - 1) // 2, 3, 3), dtype=np.uint64)
        i64p = C.POINTER(C.c_int64)
        self._check(self._L.abn_pairwise_transitions_windows_packed(
            self._h, packed.ctypes.data_as(C.POINTER(C.c_uint8)), n, int(n_sites), stride, b.ctypes.data_as(i64p),
            e.ctypes.data_as(i64p), b.shape[0], table.ctypes.data_as(C.POINTER(C.c_uint64))))
        return table

    def pairwise_transitions_windows_packed_dev(self, packed_ptr: int, n_samples: int, n_sites: int, row_stride: int,
                                                begin, end, table_ptr: int) -> float:
        """The same on device-resident buffers: packed rows [n x row_stride] (16-byte aligned) in, u64 table
        [n_windows x pairs x 9] out; begin / end are host arrays.  Returns the kernels' HIP-event ms."""
        b, e = np.ascontiguousarray(begin, dtype=np.int64), np.ascontiguousarray(end, dtype=np.int64)
        if b.ndim != 1 or b.shape != e.shape:
            raise ValueError("begin and end are 1-d arrays of one length")
        ms = C.c_double(0.0)
        i64p = C.POINTER(C.c_int64)
        self._check(self._L.abn_pairwise_transitions_windows_packed_dev(
            self._h, C.c_void_p(packed_ptr), n_samples, n_sites, row_stride, b.ctypes.data_as(i64p),
            e.ctypes.data_as(i64p), b.shape[0], C.c_void_p(table_ptr or None), C.byref(ms)))
        return ms.value

    def block_counts(self, seed: int, group_id, group_begin, group_end, n_replicates: int, n_blocks: int) -> np.ndarray:
        """The block bootstrap's counts, made on the device (abn_block_counts): uint8 (G, n_replicates + 1, n_blocks).
        Row r < n_replicates of group g is the histogram of T_g draws from the group's blocks [group_begin[g],
        group_end[g]), a function of (seed, group_id[g], r) alone; the last row is the identity row of ones; zero
        outside a group's range."""
        gid, gb, ge = _block_groups(group_begin, group_end, group_id)
        counts = np.zeros((gb.shape[0], int(n_replicates) + 1 if n_replicates >= 0 else 0, max(int(n_blocks), 0)), dtype=np.uint8)
        i64p = C.POINTER(C.c_int64)
        self._check(self._L.abn_block_counts(self._h, int(seed), gb.shape[0], _u32p(gid), gb.ctypes.data_as(i64p),
                                             ge.ctypes.data_as(i64p), int(n_replicates), int(n_blocks),
                                             counts.ctypes.data_as(C.POINTER(C.c_uint8))))
        return counts

    def block_resample(self, group_begin, group_end, counts, both, diff, level_sum_kept, kept):
        """Every row's sums over its group's blocks (abn_block_resample), exact: counts uint8 (G, rows, T) — drawn by
        block_counts, or any weights 0 .. 127 such as a jackknife's —, both / diff uint64 (T, pairs), level_sum_kept /
        kept (n, T).  Returns {both, diff, dvalue: (G, rows, pairs); level, kept: (G, rows, n)}."""
        a = _block_arguments(group_begin, group_end, counts, both, diff, level_sum_kept, kept)
        out = _block_outputs(a)
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
        i64p = C.POINTER(C.c_int64)
        ptr = [C.c_void_p(p or None) for p in (both_ptr, diff_ptr, level_ptr, kept_ptr, both_out_ptr, diff_out_ptr,
                                                 dvalue_out_ptr, level_out_ptr, kept_out_ptr)]
        self._check(self._L.abn_block_resample_dev(self._h, gb.shape[0], gb.ctypes.data_as(i64p), ge.ctypes.data_as(i64p),
                                                   int(rows_per_group), C.c_void_p(counts_ptr or None), int(n_blocks),
                                                   int(n_pairs), int(n_samples), *ptr, _dp(ms)))
        return ms

    def analyze_batch_dev(self, raw_ptr: int, n_windows: int, n_boot: int, out_ptr: int, first_bad_ptr: int = 0,
                          allow_failed_windows=False) -> float:
        """analyze_batch on device-resident buffers (raw device pointers): f64 raw [n_windows x n_boot x 7] in, f64 out
        [n_windows x 32] and i32 first_bad [n_windows] (0 = not wanted) out.  Returns the kernel's HIP-event ms."""
        ms = C.c_double(0.0)
        rc = self._L.abn_analyze_batch_dev(self._h, C.c_void_p(raw_ptr), n_windows, n_boot, C.c_void_p(out_ptr),
                                           C.c_void_p(first_bad_ptr or None), C.byref(ms))
        if not (rc == 5 and allow_failed_windows):
            self._check(rc)
        return ms.value

    def parse_sites(self, text: bytes, *, skip_lines: int = 1, slab_bytes: int = 0, contexts=("CG",)):
        """MethylationSite::from_methylome_file_line (src/methylation_site.rs:146-362) for every line of a methylome
        file's text from line skip_lines on, on the device.  Returns (sites, deferred): sites = a dict of arrays over the
        accepted sites in file order (line, chromosome, start, end, strand, posteriormax, status, status_flag, meth_lvl;
        n_lines and kernel_ms beside them); deferred = a dict of line, offset, length of the lines the device leaves to
        the host's parser (an f64 field it cannot be certain of, a line beyond its staging limit).  contexts: the
        methylation contexts whose lines are sites (names of CONTEXTS, or the mask); with any other value than CG alone
        sites gains `context`, every site's code (0 CG, 1 CHG, 2 CHH, 3 a row without one)."""
        text = bytes(text)
        mask = _context_mask(contexts)
        p = SitesParams(slab_bytes, skip_lines, 0 if mask == 1 else mask)
        h = C.c_void_p()
        self._check(self._L.abn_sites_parse(self._h, text, len(text), C.byref(p), C.byref(h)))
        s = Sites(self, h)
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
        text = bytes(text)
        mask = _context_mask(contexts)
        p = SitesParams(slab_bytes, skip_lines, 0 if mask == 1 else mask)
        h = C.c_void_p()
        self._check(self._L.abn_sites_parse_dev(self._h, text, len(text), C.byref(p), C.byref(h)))
        return Sites(self, h)

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
        u8p = C.POINTER(C.c_uint8)
        self._check(self._L.abn_genes_choose(genes._h, C.byref(rule), off.shape[0] - 1, off.ctypes.data_as(C.POINTER(C.c_int64)),
                                             u[0].ctypes.data_as(C.POINTER(C.c_int32)), _u32p(u[1]), _u32p(u[2]),
                                             u[3].ctypes.data_as(u8p), _u32p(gs), _u32p(ge), fl.ctypes.data_as(u8p), _dp(ms)))
        return gs, ge, fl, ms

    def common_sites(self, site_offset, chromosome, start, end, strand):
        """The sites every sample shares, by key (chromosome, start, end, strand), on the device (abn_sites_common: lifts
        the assumption of src/pedigree.rs:240).  Arguments as choose_genes.  Returns (keep uint8 (S,), n_common): keep marks
        every sample's common sites, n_common of them in each.  AbnError when a sample is not well ordered (a chromosome in
        two runs, a key not above the one before it) or the samples' common sites come in different orders."""
        off, u = _site_arrays(site_offset, chromosome, start, end, strand)
        keep = np.zeros(int(off[-1]), dtype=np.uint8)
        n_common = C.c_int64(-1)
        u8p = C.POINTER(C.c_uint8)
        self._check(self._L.abn_sites_common(self._h, off.shape[0] - 1, off.ctypes.data_as(C.POINTER(C.c_int64)),
                                             u[0].ctypes.data_as(C.POINTER(C.c_int32)), _u32p(u[1]), _u32p(u[2]),
                                             u[3].ctypes.data_as(u8p), keep.ctypes.data_as(u8p), C.byref(n_common)))
        return keep, n_common.value

    def sort_sites(self, chromosome, start, end, strand):
        """The stable permutation of one sample's keys into canonical order — ascending chromosome, start, end, strand — on
        the device (abn_sites_sort_keys).  Returns (order int64 (n,), info): info = {sites, descents, equal, passes} as
        Sites.sort_info.  AbnError for a chromosome outside 0..257 or a strand above 2."""
        n = np.asarray(chromosome).reshape(-1).shape[0]
        _, u = _site_arrays([0, n], chromosome, start, end, strand)
        order, info = np.zeros(n, dtype=np.int64), np.zeros(4, dtype=np.int64)
        i64p = C.POINTER(C.c_int64)
        self._check(self._L.abn_sites_sort_keys(self._h, n, u[0].ctypes.data_as(C.POINTER(C.c_int32)), _u32p(u[1]), _u32p(u[2]),
                                                u[3].ctypes.data_as(C.POINTER(C.c_uint8)), order.ctypes.data_as(i64p),
                                                info.ctypes.data_as(i64p)))
        return order, {"sites": int(info[0]), "descents": int(info[1]), "equal": int(info[2]), "passes": int(info[3])}

    def union_sites(self, site_offset, chromosome, start, end, strand):
        """The union of the samples' sites, by key (chromosome, start, end, strand), on the device (abn_sites_union: the
        per-pair comparison of src/pedigree.rs:240-254 for samples that hold different sites).  Arguments as common_sites.
        Returns (dest uint32 (S,), n_union): every site's rank in the union order, n_union distinct keys.  AbnError when a
        sample is not well ordered or its chromosomes come in another order than the union's."""
        off, u = _site_arrays(site_offset, chromosome, start, end, strand)
        dest = np.zeros(int(off[-1]), dtype=np.uint32)
        n_union = C.c_int64(-1)
        u8p = C.POINTER(C.c_uint8)
        self._check(self._L.abn_sites_union(self._h, off.shape[0] - 1, off.ctypes.data_as(C.POINTER(C.c_int64)),
                                            u[0].ctypes.data_as(C.POINTER(C.c_int32)), _u32p(u[1]), _u32p(u[2]),
                                            u[3].ctypes.data_as(u8p), _u32p(dest), C.byref(n_union)))
        return dest, n_union.value

    def choose_genes_dev(self, genes: "Genes", site_offset, chromosome_ptr: int, start_ptr: int, end_ptr: int,
                         strand_ptr: int, gene_start_ptr: int, gene_end_ptr: int, flags_ptr: int, *, cutoff,
                         cutoff_gene_length=False) -> np.ndarray:
        """choose_genes on device-resident arrays (raw device pointers; site_offset stays a host array).  Returns the
        three kernels' HIP-event ms."""
        off = np.ascontiguousarray(site_offset, dtype=np.int64)
        ms = np.zeros(3)
        rule = GeneRule(cutoff, 1 if cutoff_gene_length else 0)
        self._check(self._L.abn_genes_choose_dev(genes._h, C.byref(rule), off.shape[0] - 1,
                                                 off.ctypes.data_as(C.POINTER(C.c_int64)),
                                                 *(C.c_void_p(p or None) for p in (chromosome_ptr, start_ptr, end_ptr,
                                                                                   strand_ptr, gene_start_ptr,
                                                                                   gene_end_ptr, flags_ptr)), _dp(ms)))
        return ms

    # ---- (3) boot_model::run
    def boot_model_run(self, pedigree, model, pred, resid, p0uu, eqp, eqp_weight, n_boot, *,
                       options: Options | None = None):
        ped = _f64(pedigree).reshape(-1, 4)
        n = ped.shape[0]
        raw = np.empty((n_boot, 7))
        info = np.zeros(n_boot, dtype=FIT_INFO_DTYPE)
        self._check(self._L.abn_boot_model_run(self._h, C.byref(options) if options else None, _dp(ped), n,
                                               _dp(_f64(model, (4,))), _dp(_f64(pred, (n,))), _dp(_f64(resid, (n,))),
                                               p0uu, eqp, eqp_weight, n_boot, _dp(raw), info.ctypes.data))
        return raw, info


class _Handle:
    """A handle of the library (`_h`, made by the subclass through `_L`) and its end: `_DESTROY` names the entry point that
    frees it, called once — by close() or when the object is collected."""

    _DESTROY = ""
    _h = None

    @classmethod
    def _new(cls, ctx: "Context"):
        """an instance of ctx, its handle still to be made (the alternative constructors)"""
        self = cls.__new__(cls)
        self.ctx, self._L = ctx, ctx._L
        return self

    def close(self):
        if self._h:
            getattr(self._L, self._DESTROY)(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Plan(_Handle):
    """abn_plan: device-resident batch of W windows x (S starts + B bootstraps) over one pedigree topology."""

    _DESTROY = "abn_plan_destroy"

    def __init__(self, ctx: Context, generations, n_windows, n_starts, n_boot, *, window_offset=0, boot_offset=0,
                 options: Options | None = None):
        self.ctx = ctx
        self._L = ctx._L
        g = _f64(generations).reshape(-1, 3)
        self.N, self.W, self.S, self.B = g.shape[0], n_windows, n_starts, n_boot
        h = C.c_void_p()
        ctx._check(self._L.abn_plan_create(ctx._h, C.byref(options) if options else None, _dp(g), self.N, n_windows,
                                           n_starts, n_boot, window_offset, boot_offset, C.byref(h)))
        self._h = h

    def set_window_ids(self, ids):
        """ids[W]: every window's index in the Philox counters (default window_offset + w); before set_windows"""
        a = None if ids is None else np.ascontiguousarray(ids, dtype=np.uint32).reshape(self.W)
        self.ctx._check(self._L.abn_plan_set_window_ids(self._h, _u32p(a)))

    def failed_windows(self) -> int:
        """windows whose selection found no finite start in the last phase-A run"""
        n = C.c_int32(0)
        self.ctx._check(self._L.abn_plan_failed_windows(self._h, C.byref(n)))
        return n.value

    def set_windows(self, d_obs, p0uu, eqp=None, eqp_weight=None):
        d = _f64(d_obs, (self.W, self.N))
        p = _f64(p0uu, (self.W,))
        e = None if eqp is None else _f64(eqp, (self.W,))
        ew = None if eqp_weight is None else _f64(eqp_weight, (self.W,))
        self.ctx._check(self._L.abn_plan_set_windows(self._h, _dp(d), _dp(p), _dp(e), _dp(ew)))

    def run(self):
        self.ctx._check(self._L.abn_plan_run(self._h))

    def run_phase(self, phase: int):
        self.ctx._check(self._L.abn_plan_run_phase(self._h, phase))

    def sync(self):
        self.ctx._check(self._L.abn_plan_sync(self._h))

    def tail_handed(self):
        """chains the last persistent launch of (phase A, phase B) handed to the speculative kernel for its tail"""
        out = (C.c_int64 * 2)()
        self.ctx._check(self._L.abn_plan_tail_handed(self._h, out))
        return int(out[0]), int(out[1])

    def set_early_bootstraps(self, mode: int):
        """0: run() launches phase B after the slowest start; 1 (default): on a quorum of the starts where the plan is
        eligible (one window, >= 5 starts on the speculative kernel, bootstraps on the persistent kernel)"""
        self.ctx._check(self._L.abn_plan_set_early_bootstraps(self._h, mode))

    def early_bootstraps(self):
        """the plan's eligibility and quorum; starts parked at the quorum and the miss flag of the last run()"""
        out = (C.c_int32 * 4)()
        self.ctx._check(self._L.abn_plan_early_bootstraps(self._h, out))
        return {"eligible": bool(out[0]), "quorum": int(out[1]), "parked": int(out[2]), "miss": bool(out[3])}

    def set_stream_sweep(self, mode: int):
        """0 (default): streamed chains re-read their rows every cost evaluation; 1: once per Nelder-Mead iteration
        (reflection, expansion and contraction in one pass) where the launch streams with a wavefront per chain — same
        bytes either way"""
        self.ctx._check(self._L.abn_plan_set_stream_sweep(self._h, mode))

    def stream_sweep(self):
        """the mode; whether the last run of each phase used the sweep kernel; passes over the rows those launches counted"""
        out = (C.c_int64 * 4)()
        self.ctx._check(self._L.abn_plan_stream_sweep(self._h, out))
        return {"mode": int(out[0]), "starts": bool(out[1]), "boot": bool(out[2]), "passes": int(out[3])}

    def kernel_ms(self):
        ms = np.zeros(3)
        self.ctx._check(self._L.abn_plan_kernel_ms(self._h, _dp(ms)))
        return {"fit_starts": ms[0], "select": ms[1], "fit_boot": ms[2]}

    def raw_device_ptr(self) -> int:
        p = C.c_void_p()
        self.ctx._check(self._L.abn_plan_raw_device_ptr(self._h, C.byref(p)))
        return p.value or 0

    def bind_raw(self, dev_ptr: int):
        self.ctx._check(self._L.abn_plan_bind_raw(self._h, C.c_void_p(dev_ptr)))

    def download(self, want_info=True, allow_failed_windows=False):
        """Raises AbnError(ABN_ERR_NO_FINITE_FIT) when a window has no finite start (the reference panics) unless
        allow_failed_windows: then the dict comes back with best_start = -1 and NaN rows for those windows."""
        W, N, S, B = self.W, self.N, self.S, self.B
        models, pred, resid = np.empty((W, 4)), np.empty((W, N)), np.empty((W, N))
        raw = np.empty((W, B, 7)) if B else None
        ia = np.zeros((W, S), dtype=FIT_INFO_DTYPE) if (S and want_info) else None
        ib = np.zeros((W, B), dtype=FIT_INFO_DTYPE) if (B and want_info) else None
        bs = np.full(W, -1, dtype=np.int32)
        rc = self._L.abn_plan_download(self._h, _dp(models), _dp(pred), _dp(resid), _dp(raw),
                                       None if ia is None else ia.ctypes.data,
                                       None if ib is None else ib.ctypes.data,
                                       bs.ctypes.data_as(C.POINTER(C.c_int32)))
        if not (rc == 5 and allow_failed_windows):  # ABN_ERR_NO_FINITE_FIT: every buffer is filled all the same
            self.ctx._check(rc)
        return {"models": models, "pred": pred, "resid": resid, "raw": raw, "info_a": ia, "info_b": ib,
                "best_start": bs}

    def analyze(self, allow_failed_windows=False):
        """The analysis of every window on the device, from the table the plan currently writes (bind_raw included):
        (out (W, 32), first_bad (W,)) as analyze_batch — W x 32 doubles come back instead of raw (W, B, 7)."""
        out, fb = np.empty((self.W, 32)), np.full(self.W, -1, dtype=np.int32)
        rc = self._L.abn_plan_analyze(self._h, _dp(out), fb.ctypes.data_as(C.POINTER(C.c_int32)))
        if not (rc == 5 and allow_failed_windows):
            self.ctx._check(rc)
        return out, fb

    def counters(self):
        out = (C.c_int64 * 5)()
        self.ctx._check(self._L.abn_plan_counters(self._h, out))
        return {"fits": out[0], "evals": out[1], "iters": out[2], "evals_skipped": out[3] + out[4],
                "evals_skipped_starts": out[3], "evals_skipped_boot": out[4]}

    def device_bytes(self) -> int:
        b = C.c_int64()
        self.ctx._check(self._L.abn_plan_device_bytes(self._h, C.byref(b)))
        return b.value

    def last_kernels(self):
        """which fit kernel the last run of each phase used (ABN_KERNEL_* names) and its lanes per chain"""
        out = (C.c_int32 * 4)()
        self.ctx._check(self._L.abn_plan_last_kernels(self._h, out))
        return {"starts": (KERNEL_NAMES.get(out[0], out[0]), out[1]), "boot": (KERNEL_NAMES.get(out[2], out[2]), out[3])}


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


def _site_arrays(site_offset, chromosome, start, end, strand):
    off = np.ascontiguousarray(site_offset, dtype=np.int64)
    S = int(off[-1]) if off.shape[0] else 0
    return off, [np.ascontiguousarray(a, dtype=t).reshape(S) for a, t in
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
        self.ctx._check(self._L.abn_sites_info(self._h, C.byref(n), C.byref(nd), C.byref(nl), C.byref(ms)))
        return {"n_sites": n.value, "n_deferred": nd.value, "n_lines": nl.value, "kernel_ms": ms.value}

    def deferred(self):
        """{line, offset, length} of the lines left to the host's parser, in file order"""
        out = {k: np.zeros(self.info()["n_deferred"], dtype=np.int64) for k in ("line", "offset", "length")}
        self.ctx._check(self._L.abn_sites_deferred(self._h, *(a.ctypes.data_as(C.POINTER(C.c_int64)) for a in out.values())))
        return out

    def flagged(self) -> np.ndarray:
        """the file lines of the records whose status byte was none of M, I, U, ascending"""
        n = C.c_int64()
        self.ctx._check(self._L.abn_sites_flagged(self._h, C.byref(n), None))
        out = np.zeros(n.value, dtype=np.int64)
        self.ctx._check(self._L.abn_sites_flagged(self._h, None, out.ctypes.data_as(C.POINTER(C.c_int64))))
        return out

    def insert(self, line, chromosome, start, end, strand, posteriormax, status, meth_lvl, context=None):
        """the deferred lines the host's parser accepted, ascending by line; once per handle (abn_sites_insert).  context:
        every record's code (abn_sites_insert_ctx); None is code 0 for all, which a handle of other contexts than CG
        refuses."""
        arrays = [np.ascontiguousarray(a, dtype=t).reshape(-1) for a, t in
                  zip((line, chromosome, start, end, strand, posteriormax, status, meth_lvl),
                      (np.int64, np.int32, np.uint32, np.uint32, np.uint8, np.float64, np.uint8, np.float64))]
        call = self._L.abn_sites_insert
        if context is not None:
            arrays.append(np.ascontiguousarray(context, dtype=np.uint8).reshape(-1))
            call = self._L.abn_sites_insert_ctx
        if len({a.shape[0] for a in arrays}) != 1:
            raise ValueError("the arrays are of one length")
        self.ctx._check(call(self._h, arrays[0].shape[0], *(a.ctypes.data_as(t) for a, t in zip(arrays, call.argtypes[2:]))))

    def mask(self) -> int:
        """the contexts the handle was parsed under (1 CG, 2 CHG, 4 CHH)"""
        m = C.c_int32()
        self.ctx._check(self._L.abn_sites_context(self._h, C.byref(m), None))
        return m.value

    def contexts(self) -> np.ndarray:
        """every site's context code in the order of fetch(): 0 CG, 1 CHG, 2 CHH, 3 a row without one"""
        out = np.zeros(self.info()["n_sites"], dtype=np.uint8)
        self.ctx._check(self._L.abn_sites_context(self._h, None, out.ctypes.data_as(C.POINTER(C.c_uint8))))
        return out

    def split(self) -> "dict[str, Sites]":
        """One resident handle per context of the handle's mask, partitioned on the device (abn_sites_split): each holds
        what parse_sites_resident of the same text with that context alone, its deferred lines inserted, holds, and goes
        into Windows.from_parsed, Codes.from_parsed and Tiles as it is.  This handle stays usable."""
        out = (C.c_void_p * 3)()
        self.ctx._check(self._L.abn_sites_split(self._h, out))
        return {name: Sites(self.ctx, C.c_void_p(h)) for name, h in zip(CONTEXTS, out) if h}

    def split_ms(self):
        """(count kernel ms, scatter kernel ms) of the last split() of this handle, or of the split that made it"""
        ms = np.zeros(2)
        self.ctx._check(self._L.abn_sites_split_ms(self._h, _dp(ms)))
        return float(ms[0]), float(ms[1])

    def sort(self) -> "Sites":
        """A new resident handle with this handle's sites — device records and inserted ones — in canonical order:
        ascending chromosome key, start, end, strand, equal keys in file order (abn_sites_sort: a stable radix sort on the
        device).  Its lines are 0 .. n_sites - 1; it goes into Windows.from_parsed, Codes.from_parsed, Tiles and split() as
        it is.  This handle stays usable."""
        out = C.c_void_p()
        self.ctx._check(self._L.abn_sites_sort(self._h, C.byref(out)))
        return Sites(self.ctx, out)

    def sort_order(self) -> np.ndarray:
        """of a handle sort() made: the index, in the parent's fetch(), of every site (abn_sites_sort_order)"""
        n = C.c_int64()
        self.ctx._check(self._L.abn_sites_sort_order(self._h, C.byref(n), None))
        order = np.zeros(n.value, dtype=np.int64)
        self.ctx._check(self._L.abn_sites_sort_order(self._h, None, order.ctypes.data_as(C.POINTER(C.c_int64))))
        return order

    def sort_info(self):
        """of a handle sort() made: {sites, descents, equal (neighbours of the input), passes (radix passes run), ms: the
        HIP-event ms of flatten, check, passes, gather}"""
        info, ms = np.zeros(4, dtype=np.int64), np.zeros(4)
        self.ctx._check(self._L.abn_sites_sort_info(self._h, info.ctypes.data_as(C.POINTER(C.c_int64)), _dp(ms)))
        return {"sites": int(info[0]), "descents": int(info[1]), "equal": int(info[2]), "passes": int(info[3]), "ms": ms}

    def fetch(self):
        """the sites in file order as a dict of arrays (Context.parse_sites' fields); a resident handle downloads them and
        merges the inserted records in by line"""
        sites = {k: np.zeros(self.info()["n_sites"], dtype=t) for k, t in self.KINDS.items()}
        self.ctx._check(self._L.abn_sites_fetch(self._h, *(a.ctypes.data_as(t) for a, t in
                                                           zip(sites.values(), self._L.abn_sites_fetch.argtypes[1:]))))
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
        i32p = C.POINTER(C.c_int32)
        ctx._check(self._L.abn_genes_create(ctx._h, len(lists), chrom.ctypes.data_as(i32p), kind.ctypes.data_as(i32p),
                                            off.ctypes.data_as(C.POINTER(C.c_int64)), _u32p(start), _u32p(end),
                                            strand.ctypes.data_as(C.POINTER(C.c_uint8)), C.byref(h)))
        self._h = h
        self.n_genes = int(off[-1])


class _PackedMatrix(_Handle):
    """What Windows and Codes share: the report of the alignment they were made with, and the packed matrix
    (n_samples, row_stride) they keep on the device.  `_PREFIX` is the C prefix of their entry points."""

    _PREFIX = ""

    def _entry(self, name):
        return getattr(self._L, f"{self._PREFIX}_{name}")

    def _aligned(self, entry, n_ms):
        before, each, ms = np.zeros(self.n_samples, dtype=np.int64), C.c_int64(-1), np.zeros(n_ms)
        self.ctx._check(self._entry(entry)(self._h, before.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(each), _dp(ms)))
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
        self.ctx._check(self._entry("packed")(self._h, out.ctypes.data_as(C.POINTER(C.c_uint8))))
        return out

    def packed_device_ptr(self) -> int:
        p = C.c_void_p()
        self.ctx._check(self._entry("packed_device_ptr")(self._h, C.byref(p)))
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
        off = np.ascontiguousarray(site_offset, dtype=np.int64)
        self.n_samples = off.shape[0] - 1
        S = int(off[-1]) if off.shape[0] else 0
        u32 = [np.ascontiguousarray(a, dtype=np.uint32).reshape(S) for a in (pos, gene_start, gene_end)]
        u8 = [np.ascontiguousarray(a, dtype=np.uint8).reshape(S) for a in (flags, code)]
        lvl = _f64(level, (S,))
        p = WindowsParams(cutoff, step, size, 1 if absolute else 0, *map(int, counts))
        h = C.c_void_p()
        u8p = C.POINTER(C.c_uint8)
        ctx._check(self._L.abn_windows_create(ctx._h, C.byref(p), self.n_samples, off.ctypes.data_as(C.POINTER(C.c_int64)),
                                              _u32p(u32[0]), _u32p(u32[1]), _u32p(u32[2]), u8[0].ctypes.data_as(u8p),
                                              u8[1].ctypes.data_as(u8p), _dp(lvl), C.byref(h)))
        self._finish(h)

    def _finish(self, h):
        """the handle taken, and what abn_windows_info says of it"""
        self._h = h
        W, stride, ns = C.c_int32(), C.c_int64(), C.c_int64()
        self.ctx._check(self._L.abn_windows_info(h, C.byref(W), C.byref(stride), C.byref(ns)))
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
        co = np.ascontiguousarray(code, dtype=np.uint8).reshape(S)
        lvl = _f64(level, (S,))
        p = WindowsParams(cutoff, step, size, 1 if absolute else 0, *map(int, counts))
        rule = GeneRule(cutoff, 1 if cutoff_gene_length else 0)
        h = C.c_void_p()
        u8p = C.POINTER(C.c_uint8)
        ctx._check(self._L.abn_windows_create_sites(ctx._h, C.byref(p), genes._h, C.byref(rule), self.n_samples,
                                                    off.ctypes.data_as(C.POINTER(C.c_int64)),
                                                    u[0].ctypes.data_as(C.POINTER(C.c_int32)), _u32p(u[1]), _u32p(u[2]),
                                                    u[3].ctypes.data_as(u8p), co.ctypes.data_as(u8p), _dp(lvl), C.byref(h)))
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
        sites_list = list(sites_list)
        self.n_samples = len(sites_list)
        p = WindowsParams(cutoff, step, size, 1 if absolute else 0, *map(int, counts))
        rule = GeneRule(cutoff, 1 if cutoff_gene_length else 0)
        handles = (C.c_void_p * max(self.n_samples, 1))(*(s._h for s in sites_list))
        h = C.c_void_p()
        create = getattr(self._L, _ALIGN_CREATE[_align_mode(align)].format("windows"))
        ctx._check(create(ctx._h, C.byref(p), genes._h, C.byref(rule), posterior_max_filter, self.n_samples, handles,
                          C.byref(h)))
        return self._finish(h)

    def merge_ms(self) -> np.ndarray:
        """the HIP-event ms of from_parsed's two merge kernels (fields, insert); zeros for the other forms"""
        ms = np.zeros(2)
        self.ctx._check(self._L.abn_windows_merge_ms(self._h, _dp(ms)))
        return ms

    def stats(self):
        """(count int64, level_sum, level_sum_kept, kept int64), each (n_samples, W)"""
        shape = (self.n_samples, self.W)
        count, kept = np.zeros(shape, dtype=np.int64), np.zeros(shape, dtype=np.int64)
        ls, lsk = np.zeros(shape), np.zeros(shape)
        i64p = C.POINTER(C.c_int64)
        self.ctx._check(self._L.abn_windows_stats(self._h, count.ctypes.data_as(i64p), _dp(ls), _dp(lsk),
                                                  kept.ctypes.data_as(i64p)))
        return count, ls, lsk, kept

    def layout(self):
        """(begin int64, end int64, ragged int32), each (W,): window w = the fields [begin[w], end[w]) of every row"""
        b, e = np.zeros(self.W, dtype=np.int64), np.zeros(self.W, dtype=np.int64)
        r = np.zeros(self.W, dtype=np.int32)
        i64p = C.POINTER(C.c_int64)
        self.ctx._check(self._L.abn_windows_layout(self._h, b.ctypes.data_as(i64p), e.ctypes.data_as(i64p),
                                                   r.ctypes.data_as(C.POINTER(C.c_int32))))
        return b, e, r

    def pairwise(self):
        """(diff, both, dvalue), each (W, pairs): pairwise_divergence of every window, on the resident matrix"""
        npairs = self.n_samples * (self.n_samples - 1) // 2
        diff, both = np.zeros((self.W, npairs), dtype=np.uint64), np.zeros((self.W, npairs), dtype=np.uint64)
        dval = np.zeros((self.W, npairs))
        u64p = C.POINTER(C.c_uint64)
        self.ctx._check(self._L.abn_windows_pairwise(self._h, diff.ctypes.data_as(u64p), both.ctypes.data_as(u64p),
                                                     _dp(dval)))
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
        sites_list = list(sites_list)
        handles = (C.c_void_p * max(len(sites_list), 1))(*(s._h for s in sites_list))
        h = C.c_void_p()
        create = getattr(self._L, _ALIGN_CREATE[_align_mode(align)].format("codes"))
        ctx._check(create(ctx._h, posterior_max_filter, len(sites_list), handles, C.byref(h)))
        self._h = h
        i = self.info()
        self.n_samples, self.n_sites, self.row_stride, self.same_len = i["n_samples"], i["n_sites"], i["row_stride"], i["same_len"]
        return self

    def info(self):
        """{n_samples, n_sites (of the longest sample), row_stride (bytes), same_len (bool)}"""
        n, same, ns, stride = C.c_int32(), C.c_int32(), C.c_int64(), C.c_int64()
        self.ctx._check(self._L.abn_codes_info(self._h, C.byref(n), C.byref(ns), C.byref(stride), C.byref(same)))
        return {"n_samples": n.value, "n_sites": ns.value, "row_stride": stride.value, "same_len": bool(same.value)}

    def stats(self):
        """(count int64, level_sum_kept, kept int64), each (n_samples,): a sample's sites, and the sum and number of the
        levels whose posterior passes the filter (rc_meth_lvl = level_sum_kept / kept)"""
        count, kept = np.zeros(self.n_samples, dtype=np.int64), np.zeros(self.n_samples, dtype=np.int64)
        lsk = np.zeros(self.n_samples)
        i64p = C.POINTER(C.c_int64)
        self.ctx._check(self._L.abn_codes_stats(self._h, count.ctypes.data_as(i64p), _dp(lsk), kept.ctypes.data_as(i64p)))
        return count, lsk, kept

    def pairwise(self):
        """(diff, both, dvalue), each (pairs,): pairwise_divergence_packed on the resident matrix; refused (AbnError) when
        the samples differ in length"""
        npairs = self.n_samples * (self.n_samples - 1) // 2
        diff, both, dval = np.zeros(npairs, dtype=np.uint64), np.zeros(npairs, dtype=np.uint64), np.zeros(npairs)
        u64p = C.POINTER(C.c_uint64)
        self.ctx._check(self._L.abn_codes_pairwise(self._h, diff.ctypes.data_as(u64p), both.ctypes.data_as(u64p), _dp(dval)))
        return diff, both, dval

    def transitions(self):
        """uint64 (pairs, 3, 3): Context.pairwise_transitions_packed on the resident matrix (under a union alignment the
        placeholder sites count in no entry); refused (AbnError) when the samples differ in length"""
        table = np.zeros((self.n_samples * (self.n_samples - 1) // 2, 3, 3), dtype=np.uint64)
        self.ctx._check(self._L.abn_codes_transitions(self._h, table.ctypes.data_as(C.POINTER(C.c_uint64))))
        return table

    def kernel_ms(self) -> np.ndarray:
        """the HIP-event ms of from_parsed's kernels: merge of the records, merge of the inserted lines, pack, fold"""
        ms = np.zeros(4)
        self.ctx._check(self._L.abn_codes_kernel_ms(self._h, _dp(ms)))
        return ms


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
        sites_list = list(sites_list)
        handles = (C.c_void_p * max(len(sites_list), 1))(*(s._h for s in sites_list))
        h = C.c_void_p()
        ctx._check(self._L.abn_tiles_create(ctx._h, posterior_max_filter, cls.ALIGN[_align_mode(align)], len(sites_list),
                                            handles, C.byref(h)))
        self._h = h
        i = self.info()
        self.n_samples, self.n_columns, self.row_stride, self.n_runs = i["n_samples"], i["n_columns"], i["row_stride"], i["n_runs"]
        return self

    def info(self):
        """{n_samples, n_columns, row_stride (bytes), n_runs, n_tiles (-1 before set_intervals / set_fixed)}"""
        n, runs, cols, stride, tiles = C.c_int32(), C.c_int32(), C.c_int64(), C.c_int64(), C.c_int64()
        self.ctx._check(self._L.abn_tiles_info(self._h, C.byref(n), C.byref(cols), C.byref(stride), C.byref(runs), C.byref(tiles)))
        return {"n_samples": n.value, "n_columns": cols.value, "row_stride": stride.value, "n_runs": runs.value,
                "n_tiles": tiles.value}

    def runs(self):
        """(chromosome int32, first int64, count int64, last_start uint32), each (n_runs,): the chromosome runs of the
        columns in run order, and the start of every run's last column"""
        chrom, last = np.zeros(self.n_runs, dtype=np.int32), np.zeros(self.n_runs, dtype=np.uint32)
        first, count = np.zeros(self.n_runs, dtype=np.int64), np.zeros(self.n_runs, dtype=np.int64)
        i64p = C.POINTER(C.c_int64)
        self.ctx._check(self._L.abn_tiles_runs(self._h, chrom.ctypes.data_as(C.POINTER(C.c_int32)), first.ctypes.data_as(i64p),
                                               count.ctypes.data_as(i64p), _u32p(last)))
        return chrom, first, count, last

    def set_intervals(self, chromosome, start, end):
        """the tiles (chromosome 0..257, start, end), half-open on a site's start, bounds in [0, 2^32]: the search and the
        per-(sample, tile) folds run on the device; a new list replaces the old"""
        chrom = np.ascontiguousarray(chromosome, dtype=np.int32).ravel()
        lo, hi = (np.ascontiguousarray(a, dtype=np.int64).ravel() for a in (start, end))
        if not chrom.shape == lo.shape == hi.shape:
            raise ValueError("chromosome, start and end differ in length")
        i64p = C.POINTER(C.c_int64)
        self.ctx._check(self._L.abn_tiles_set_intervals(self._h, chrom.shape[0], chrom.ctypes.data_as(C.POINTER(C.c_int32)),
                                                        lo.ctypes.data_as(i64p), hi.ctypes.data_as(i64p)))

    def set_fixed(self, size, step=0):
        """fixed tiles: for every run in run order [k step, k step + size), k = 0 .. ceil((last_start + 1) / step) - 1
        (step 0: size)"""
        self.ctx._check(self._L.abn_tiles_set_fixed(self._h, int(size), int(step)))

    def set_pools(self, chromosome, start, end, pool, n_pools):
        """pools of intervals (abn_tiles_set_pools): interval k belongs to pool[k] in [0, n_pools); a pool's columns are
        those inside at least one of its intervals, each once, in column order, gathered into a pooled matrix on the
        device.  Afterwards the tiles are the pools: layout() is in pooled column space, stats() and pairwise() per pool"""
        chrom, ids = (np.ascontiguousarray(a, dtype=np.int32).ravel() for a in (chromosome, pool))
        lo, hi = (np.ascontiguousarray(a, dtype=np.int64).ravel() for a in (start, end))
        if not chrom.shape == lo.shape == hi.shape == ids.shape:
            raise ValueError("chromosome, start, end and pool differ in length")
        i32p, i64p = C.POINTER(C.c_int32), C.POINTER(C.c_int64)
        self.ctx._check(self._L.abn_tiles_set_pools(self._h, chrom.shape[0], chrom.ctypes.data_as(i32p), lo.ctypes.data_as(i64p),
                                                    hi.ctypes.data_as(i64p), ids.ctypes.data_as(i32p), int(n_pools)))

    def pool_segments(self):
        """(pool int32, chromosome int32, start int64, end int64, col_begin int64, col_end int64), each (n_segments,): the
        pools' merged intervals in segment order and their columns of the handle's own matrix"""
        n = C.c_int64()
        self.ctx._check(self._L.abn_tiles_pool_segments(self._h, C.byref(n), None, None, None, None, None, None))
        pool, chrom = np.zeros(n.value, dtype=np.int32), np.zeros(n.value, dtype=np.int32)
        lo, hi, cb, ce = (np.zeros(n.value, dtype=np.int64) for _ in range(4))
        i32p, i64p = C.POINTER(C.c_int32), C.POINTER(C.c_int64)
        self.ctx._check(self._L.abn_tiles_pool_segments(self._h, None, pool.ctypes.data_as(i32p), chrom.ctypes.data_as(i32p),
                                                        *(a.ctypes.data_as(i64p) for a in (lo, hi, cb, ce))))
        return pool, chrom, lo, hi, cb, ce

    def pool_columns(self):
        """int64 (pooled columns,): every pooled column's source column of the handle's own matrix"""
        self.ctx._check(self._L.abn_tiles_pool_segments(self._h, None, None, None, None, None, None, None))   # pools, or refused
        end = self.layout()[1]
        src = np.zeros(int(end[-1]) if len(end) else 0, dtype=np.int64)
        self.ctx._check(self._L.abn_tiles_pool_columns(self._h, src.ctypes.data_as(C.POINTER(C.c_int64))))
        return src

    def pool_kernel_ms(self) -> np.ndarray:
        """the HIP-event ms of the last set_pools: offsets, map, gather, pack (search and fold: kernel_ms)"""
        ms = np.zeros(4)
        self.ctx._check(self._L.abn_tiles_pool_kernel_ms(self._h, _dp(ms)))
        return ms

    def _n_tiles(self):
        return max(self.info()["n_tiles"], 0)

    def intervals(self):
        """(chromosome int32, start int64, end int64), each (n_tiles,)"""
        T = self._n_tiles()
        chrom, lo, hi = np.zeros(T, dtype=np.int32), np.zeros(T, dtype=np.int64), np.zeros(T, dtype=np.int64)
        i64p = C.POINTER(C.c_int64)
        self.ctx._check(self._L.abn_tiles_intervals(self._h, chrom.ctypes.data_as(C.POINTER(C.c_int32)),
                                                    lo.ctypes.data_as(i64p), hi.ctypes.data_as(i64p)))
        return chrom, lo, hi

    def layout(self):
        """(begin int64, end int64), each (n_tiles,): every tile's columns [begin, end)"""
        T = self._n_tiles()
        begin, end = np.zeros(T, dtype=np.int64), np.zeros(T, dtype=np.int64)
        i64p = C.POINTER(C.c_int64)
        self.ctx._check(self._L.abn_tiles_layout(self._h, begin.ctypes.data_as(i64p), end.ctypes.data_as(i64p)))
        return begin, end

    def stats(self):
        """(count int64 (n_tiles,), level_sum_kept (n_samples, n_tiles), kept int64 (n_samples, n_tiles)): a tile's columns,
        and per sample the sum and number of the tile's levels whose posterior passes the filter"""
        T = self._n_tiles()
        count, kept = np.zeros(T, dtype=np.int64), np.zeros((self.n_samples, T), dtype=np.int64)
        lsk = np.zeros((self.n_samples, T))
        i64p = C.POINTER(C.c_int64)
        self.ctx._check(self._L.abn_tiles_stats(self._h, count.ctypes.data_as(i64p), _dp(lsk), kept.ctypes.data_as(i64p)))
        return count, lsk, kept

    def pairwise(self):
        """(diff, both, dvalue), each (n_tiles, pairs): pairwise_divergence_windows_packed on the resident matrix over the
        tiles' columns"""
        T, npairs = self._n_tiles(), self.n_samples * (self.n_samples - 1) // 2
        diff, both = np.zeros((T, npairs), dtype=np.uint64), np.zeros((T, npairs), dtype=np.uint64)
        dval = np.zeros((T, npairs))
        u64p = C.POINTER(C.c_uint64)
        self.ctx._check(self._L.abn_tiles_pairwise(self._h, diff.ctypes.data_as(u64p), both.ctypes.data_as(u64p), _dp(dval)))
        return diff, both, dval

    def transitions(self):
        """uint64 (n_tiles, pairs, 3, 3): Context.pairwise_transitions_windows_packed on the resident matrix over the
        tiles' columns (with pools set: the pooled matrix, one table per pool)"""
        table = np.zeros((self._n_tiles(), self.n_samples * (self.n_samples - 1) // 2, 3, 3), dtype=np.uint64)
        self.ctx._check(self._L.abn_tiles_transitions(self._h, table.ctypes.data_as(C.POINTER(C.c_uint64))))
        return table

    def kernel_ms(self) -> np.ndarray:
        """the HIP-event ms of the last set_intervals / set_fixed: search, fold"""
        ms = np.zeros(2)
        self.ctx._check(self._L.abn_tiles_kernel_ms(self._h, _dp(ms)))
        return ms

    def block_groups(self):
        """(group_begin, group_end) of block_bootstrap's groups in block space (abn_tiles_block_groups): with pools set every
        pool's segments (in pool_segments order), else the one group of all tiles"""
        G = C.c_int64()
        self.ctx._check(self._L.abn_tiles_block_groups(self._h, C.byref(G), None, None, None))
        gb, ge = np.zeros(G.value, dtype=np.int64), np.zeros(G.value, dtype=np.int64)
        i64p = C.POINTER(C.c_int64)
        self.ctx._check(self._L.abn_tiles_block_groups(self._h, None, None, gb.ctypes.data_as(i64p), ge.ctypes.data_as(i64p)))
        return gb, ge

    def block_bootstrap(self, seed: int, n_replicates: int):
        """The block bootstrap of the handle's tiles (abn_tiles_block_bootstrap): the blocks — a pooled handle's merged
        segments, one group per pool, or the fixed, non-overlapping tiles in one group — drawn with replacement
        n_replicates times per group; refused on tiles that may overlap.  Returns {both, diff, dvalue: (G, n_replicates +
        1, pairs); level, kept: (G, n_replicates + 1, n_samples)}; the last row of a group is the observed data."""
        G = len(self.block_groups()[0])
        rows, P, n = max(int(n_replicates) + 1, 0), self.n_samples * (self.n_samples - 1) // 2, self.n_samples
        out = {"both": np.zeros((G, rows, P), dtype=np.uint64), "diff": np.zeros((G, rows, P), dtype=np.uint64),
               "dvalue": np.zeros((G, rows, P)), "level": np.zeros((G, rows, n)), "kept": np.zeros((G, rows, n), dtype=np.int64)}
        u64p, i64p = C.POINTER(C.c_uint64), C.POINTER(C.c_int64)
        self.ctx._check(self._L.abn_tiles_block_bootstrap(self._h, int(seed), int(n_replicates), out["both"].ctypes.data_as(u64p),
                                                          out["diff"].ctypes.data_as(u64p), _dp(out["dvalue"]), _dp(out["level"]),
                                                          out["kept"].ctypes.data_as(i64p)))
        return out

    def block_ms(self) -> np.ndarray:
        """the HIP-event ms of the last block_bootstrap: counts, digits, product, finish, levels"""
        ms = np.zeros(5)
        self.ctx._check(self._L.abn_tiles_block_ms(self._h, _dp(ms)))
        return ms


def _block_groups(group_begin, group_end, group_id=None):
    gb, ge = (np.ascontiguousarray(a, dtype=np.int64).ravel() for a in (group_begin, group_end))
    gid = np.arange(gb.shape[0], dtype=np.uint32) if group_id is None else np.ascontiguousarray(group_id, dtype=np.uint32).ravel()
    if not gb.shape == ge.shape == gid.shape:
        raise ValueError("group_id, group_begin and group_end differ in length")
    return gid, gb, ge


def _block_arguments(group_begin, group_end, counts, both, diff, level_sum_kept, kept):
    _, gb, ge = _block_groups(group_begin, group_end)
    counts = np.ascontiguousarray(counts, dtype=np.uint8)
    both, diff = np.ascontiguousarray(both, dtype=np.uint64), np.ascontiguousarray(diff, dtype=np.uint64)
    lsk, kept = _f64(level_sum_kept), np.ascontiguousarray(kept, dtype=np.int64)
    if counts.ndim != 3 or counts.shape[0] != gb.shape[0]:
        raise ValueError("counts is (groups, rows, blocks)")
    T = counts.shape[2]
    if both.ndim != 2 or both.shape != diff.shape or both.shape[0] != T:
        raise ValueError("both and diff are (blocks, pairs)")
    if lsk.ndim != 2 or lsk.shape != kept.shape or lsk.shape[1] != T:
        raise ValueError("level_sum_kept and kept are (samples, blocks)")
    return {"gb": gb, "ge": ge, "counts": counts, "both": both, "diff": diff, "lsk": lsk, "kept": kept}


def _block_outputs(a):
    G, rows, _ = a["counts"].shape
    P, n = a["both"].shape[1], a["lsk"].shape[0]
    return {"both": np.zeros((G, rows, P), dtype=np.uint64), "diff": np.zeros((G, rows, P), dtype=np.uint64),
            "dvalue": np.zeros((G, rows, P)), "level": np.zeros((G, rows, n)), "kept": np.zeros((G, rows, n), dtype=np.int64)}


def _block_pointers(a, out):
    """the arguments abn_block_resample and abn_block_resample_host share, behind the context"""
    i64p, u64p, u8p = C.POINTER(C.c_int64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint8)
    G, rows, T = a["counts"].shape
    return (G, a["gb"].ctypes.data_as(i64p), a["ge"].ctypes.data_as(i64p), rows, a["counts"].ctypes.data_as(u8p), T,
            a["both"].shape[1], a["lsk"].shape[0], a["both"].ctypes.data_as(u64p), a["diff"].ctypes.data_as(u64p),
            _dp(a["lsk"]), a["kept"].ctypes.data_as(i64p), out["both"].ctypes.data_as(u64p), out["diff"].ctypes.data_as(u64p),
            _dp(out["dvalue"]), _dp(out["level"]), out["kept"].ctypes.data_as(i64p))


def block_resample_host(group_begin, group_end, counts, both, diff, level_sum_kept, kept):
    """Context.block_resample in its serial host form (abn_block_resample_host): no device needed; the same refusals"""
    a = _block_arguments(group_begin, group_end, counts, both, diff, level_sum_kept, kept)
    out = _block_outputs(a)
    text = C.create_string_buffer(256)
    rc = load_library().abn_block_resample_host(*_block_pointers(a, out), text, len(text))
    if rc:
        raise AbnError(rc, text.value.decode())
    return out


def block_counts_host(seed: int, group_id, group_begin, group_end, n_replicates: int, n_blocks: int) -> np.ndarray:
    """Context.block_counts in its serial host form (abn_block_counts_host): no device needed; the same refusals"""
    gid, gb, ge = _block_groups(group_begin, group_end, group_id)
    counts = np.zeros((gb.shape[0], int(n_replicates) + 1 if n_replicates >= 0 else 0, max(int(n_blocks), 0)), dtype=np.uint8)
    i64p = C.POINTER(C.c_int64)
    text = C.create_string_buffer(256)
    rc = load_library().abn_block_counts_host(int(seed), gb.shape[0], _u32p(gid), gb.ctypes.data_as(i64p), ge.ctypes.data_as(i64p),
                                              int(n_replicates), int(n_blocks), counts.ctypes.data_as(C.POINTER(C.c_uint8)),
                                              text, len(text))
    if rc:
        raise AbnError(rc, text.value.decode())
    return counts


_host_lib = None


def load_host_library():
    """libabneutral_host.so: the C++ host layer's serial forms (host/host_capi.cpp), built beside the HIP library"""
    global _host_lib
    if _host_lib is None:
        from . import build as _build
        if not _build.PEDIGREE_LIB.exists():
            _build.build_host()
        _host_lib = C.CDLL(str(_build.PEDIGREE_LIB))
    return _host_lib


def sort_sites_host(chromosome, start, end, strand):
    """Context.sort_sites in its serial host form (abn_sites_sort_keys_host): no device needed; the same refusals, and
    info's passes = the radix passes the device would run"""
    n = np.asarray(chromosome).reshape(-1).shape[0]
    _, u = _site_arrays([0, n], chromosome, start, end, strand)
    order, info = np.zeros(n, dtype=np.int64), np.zeros(4, dtype=np.int64)
    H = load_host_library()
    H.abn_sites_sort_keys_host.argtypes = [C.c_longlong] + [C.c_void_p] * 6
    rc = H.abn_sites_sort_keys_host(n, *(a.ctypes.data for a in (*u, order, info)))
    if rc:
        raise AbnError(rc, "a chromosome outside 0..257 or a strand above 2")
    return order, {"sites": int(info[0]), "descents": int(info[1]), "equal": int(info[2]), "passes": int(info[3])}


def reduction_tree(generations, options: Options | None = None) -> int:
    """The residual reduction tree of a pedigree (abn_fit_info.lanes): host arithmetic, no device needed."""
    g = _f64(generations).reshape(-1, 3)
    t = C.c_int32(0)
    rc = load_library().abn_reduction_tree(C.byref(options) if options else None, _dp(g), g.shape[0], C.byref(t))
    if rc:
        raise AbnError(rc)
    return t.value


def multi_plan_shard(n_windows: int, n_boot: int, n_devices: int, device_index: int):
    """(window_offset, n_windows, boot_offset, n_boot) of one device's shard in the one-process / several-GPUs entry
    points (abn_multi_plan_shard: host arithmetic, no device needed)."""
    out = (C.c_int32 * 4)()
    rc = load_library().abn_multi_plan_shard(n_windows, n_boot, n_devices, device_index, out)
    if rc:
        raise AbnError(rc)
    return tuple(int(v) for v in out)


def rccl_available() -> bool:
    ok = C.c_int(0)
    load_library().abn_multi_rccl_available(C.byref(ok))
    return bool(ok.value)


class MultiPlan(_Handle):
    """abn_multi: one process, several GPUs — a plan per device, windows (or, with fewer windows than devices,
    bootstraps) sharded in contiguous blocks, the bootstrap tables gathered with RCCL over xGMI."""

    _DESTROY = "abn_multi_destroy"

    def __init__(self, devices, generations, n_windows, n_starts, n_boot, *, options: Options | None = None):
        self._L = load_library()
        g = _f64(generations).reshape(-1, 3)
        self.devices = [int(d) for d in devices]
        self.N, self.W, self.S, self.B = g.shape[0], n_windows, n_starts, n_boot
        devs = (C.c_int32 * len(self.devices))(*self.devices)
        h = C.c_void_p()
        rc = self._L.abn_multi_create(devs, len(self.devices), C.byref(options) if options else None, _dp(g), self.N,
                                      n_windows, n_starts, n_boot, C.byref(h))
        self._h = h if h.value else None
        if rc:
            msg = (self._L.abn_multi_last_error(h) or b"").decode() if h.value else ""
            self.close()
            raise AbnError(rc, msg)

    def _check(self, rc):
        if rc:
            raise AbnError(rc, (self._L.abn_multi_last_error(self._h) or b"").decode())

    def set_window_ids(self, ids):
        a = None if ids is None else np.ascontiguousarray(ids, dtype=np.uint32).reshape(self.W)
        self._check(self._L.abn_multi_set_window_ids(self._h, _u32p(a)))

    def set_stream_sweep(self, mode: int):
        """Plan.set_stream_sweep on every device's plan"""
        self._check(self._L.abn_multi_set_stream_sweep(self._h, mode))

    def set_windows(self, d_obs, p0uu, eqp=None, eqp_weight=None):
        d = _f64(d_obs, (self.W, self.N))
        p = _f64(p0uu, (self.W,))
        e = None if eqp is None else _f64(eqp, (self.W,))
        ew = None if eqp_weight is None else _f64(eqp_weight, (self.W,))
        self._check(self._L.abn_multi_set_windows(self._h, _dp(d), _dp(p), _dp(e), _dp(ew)))

    def run(self):
        self._check(self._L.abn_multi_run(self._h))

    def sync(self):
        self._check(self._L.abn_multi_sync(self._h))

    def kernel_ms(self, device_index: int = 0):
        ms = np.zeros(3)
        self._check(self._L.abn_multi_kernel_ms(self._h, device_index, _dp(ms)))
        return {"fit_starts": ms[0], "select": ms[1], "fit_boot": ms[2]}

    def shard(self, device_index: int):
        out = (C.c_int32 * 4)()
        self._check(self._L.abn_multi_shard(self._h, device_index, out))
        return {"window_offset": out[0], "n_windows": out[1], "boot_offset": out[2], "n_boot": out[3]}

    def download(self, want_info=True, allow_failed_windows=False):
        W, N, S, B = self.W, self.N, self.S, self.B
        models, pred, resid = np.empty((W, 4)), np.empty((W, N)), np.empty((W, N))
        raw = np.empty((W, B, 7))
        ia = np.zeros((W, S), dtype=FIT_INFO_DTYPE) if want_info else None
        ib = np.zeros((W, B), dtype=FIT_INFO_DTYPE) if want_info else None
        bs = np.full(W, -1, dtype=np.int32)
        rc = self._L.abn_multi_download(self._h, _dp(models), _dp(pred), _dp(resid), _dp(raw),
                                        None if ia is None else ia.ctypes.data,
                                        None if ib is None else ib.ctypes.data,
                                        bs.ctypes.data_as(C.POINTER(C.c_int32)))
        if not (rc == 5 and allow_failed_windows):
            self._check(rc)
        return {"models": models, "pred": pred, "resid": resid, "raw": raw, "info_a": ia, "info_b": ib,
                "best_start": bs}

    def analyze(self, allow_failed_windows=False):
        """Plan.analyze for all W windows, on the first device's gathered table: (out (W, 32), first_bad (W,))"""
        out, fb = np.empty((self.W, 32)), np.full(self.W, -1, dtype=np.int32)
        rc = self._L.abn_multi_analyze(self._h, _dp(out), fb.ctypes.data_as(C.POINTER(C.c_int32)))
        if not (rc == 5 and allow_failed_windows):
            self._check(rc)
        return out, fb

    def counters(self):
        out = (C.c_int64 * 5)()
        self._check(self._L.abn_multi_counters(self._h, out))
        return {"fits": out[0], "evals": out[1], "iters": out[2], "evals_skipped": out[3] + out[4],
                "evals_skipped_starts": out[3], "evals_skipped_boot": out[4]}
