"""alphabeta_rs_amd — MI355X-native ABneutral hot path (ctypes binding of the C-ABI in include/abneutral.h).

The compute path is libabneutral_hip.so (hand-written HIP for gfx950).  There is no CPU fallback: if the
library is missing or no HIP device is usable, calls raise.  PyTorch is used by callers only for
`torch.distributed` (RCCL) and stream plumbing, never for the arithmetic.

Python-level names mirror the reference crate: `Pedigree`, `Model`, `ab_neutral.run`, `boot_model.run`.  The binding
is one module per handle family — _ffi (prototypes, loaders, helpers), context, plan, sites, matrices, blocks — and this
module re-exports their names; alphabeta_rs_amd.dedup (the collapse of repeated sites) is a module of functions, imported
by its own name.
"""
from ._ffi import (ABN_OK, EXPORTED_SYMBOLS, FIT_CONVERGED, FIT_INFO_DTYPE, FIT_MAX_ITERS, FIT_NONFINITE, FIT_TARGET,
                   KERNEL_NAMES, LIB_PATH, PKG, STATUS_NAMES, AbnError, GeneRule, Options, SitesParams, WindowsParams,
                   load_host_library, load_library)
from .blocks import block_counts_host, block_resample_host
from .context import (Context, analyze, analyze_batch, default_options, device_count, gen_boot_simplices,
                      gen_start_simplices, pack_codes, packed_row_stride, unpack_codes)
from .matrices import Codes, Tiles, Windows
from .plan import MultiPlan, Plan, multi_plan_shard, rccl_available, reduction_tree
from .sites import CONTEXTS, Genes, Sites, _context_mask, sort_sites_host
