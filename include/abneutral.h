/*
 * abneutral.h — C-ABI of the MI355X-native ABneutral hot path (libabneutral_hip.so).
 *
 * Drop-in boundary for alphabeta-rs v0.2.1 (citations relative to the reference tree).  The reference
 * has no FFI layer; the seams this library sits behind are Rust-level:
 *   (1) `impl CostFunction for Problem`          src/structs.rs:191-217      -> abn_cost_batch
 *   (2) `ab_neutral::run`                        src/ab_neutral.rs:13-20     -> abn_ab_neutral_run
 *   (3) `boot_model::run`                        src/boot_model.rs:17-28     -> abn_boot_model_run
 *   (4) the serial window loop of `metaprofile`  src/cli/metaprofile.rs:50-72 -> abn_plan_* (batched)
 * INTEGRATION.md shows the `extern "C"` block + safe wrappers a maintainer would add on the Rust side.
 *
 * Conventions: plain pointers and sizes, all f64 unless noted, row-major, caller owns every buffer it
 * passes; the library owns device memory behind the opaque handles.  No exceptions cross the ABI and
 * nothing aborts: every entry point returns an abn_status (0 = ok).  A handle is thread-compatible
 * (one thread at a time); there is no hidden global state.
 *
 * There is NO CPU fallback: without a HIP device every compute entry point returns ABN_ERR_NO_DEVICE.
 */
#ifndef ABNEUTRAL_H
#define ABNEUTRAL_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ABN_VERSION_MAJOR 0
#define ABN_VERSION_MINOR 1

typedef enum abn_status {
  ABN_OK = 0,
  ABN_ERR_INVALID_ARG = 1,   /* null pointer, non-positive size, unsupported option value; also a pedigree
                                whose power table and distinct-triple list (10 (T+1) + K + 4 doubles per chain) do
                                not fit the 160 KiB of LDS a workgroup can have: K up to ~17 000 distinct triples
                                at T = 255 (64 KiB per workgroup with an explicit lanes_per_chain below 64)          */
  ABN_ERR_BAD_PEDIGREE = 2,  /* a generation outside 0..127 after the `as i8` cast, or t1/t2 < t0      */
  ABN_ERR_NO_DEVICE = 3,     /* no usable HIP device (the product path never falls back to the CPU)    */
  ABN_ERR_HIP = 4,           /* a HIP runtime call failed; see abn_last_error()                        */
  ABN_ERR_NO_FINITE_FIT = 5, /* every start of a window ended non-finite (reference: panic, :28,:100)  */
  ABN_ERR_STATE = 6          /* plan used out of order (e.g. run before set_windows)                   */
} abn_status;

/* per-fit termination status, written in fit order (no push-under-lock as in src/ab_neutral.rs:74) */
#define ABN_FIT_CONVERGED 0  /* SD of the 5 simplex costs < sd_tolerance (argmin SolverConverged)     */
#define ABN_FIT_MAX_ITERS 1  /* iteration budget reached (argmin MaxItersReached)                     */
#define ABN_FIT_NONFINITE 2  /* no finite best parameter vector (reference: `.unwrap()` panic)        */
#define ABN_FIT_TARGET 3     /* best cost <= -inf (argmin TargetCostReached with default target)      */

typedef struct abn_ctx abn_ctx;
typedef struct abn_plan abn_plan;

typedef struct abn_options {
  uint64_t seed;                        /* Philox4x32-10 key (reference: unseeded thread_rng)           */
  int32_t lanes_per_chain;              /* 0 = auto; 8, 16, 32 or 64: accumulators of the residual reduction
                                           tree = lanes per chain of the packed kernels.  Auto picks it from the
                                           PEDIGREE alone (rows, generations, distinct triples) — never from the
                                           number of fits in the launch — so results are independent of batch size
                                           and of how a job is sharded over GPUs; few-chain launches use one (or
                                           four) wavefronts per chain and reproduce the same tree bit for bit     */
  int32_t strict_order;                 /* 1 = every cost sums its residuals serially in row order, the reference's
                                           `square_sum += ...` (src/structs.rs:206-213): cost AND fit entry points,
                                           bit-equal to the oracle's lanes = 1; abn_fit_info.lanes reports 1.
                                           0 = auto: serial for pedigrees of up to 16 rows (free there; the bundled
                                           data/ pedigree is then in the reference's order by default), else the
                                           pedigree's reduction tree.  -1 = the tree whatever the size.  Like the
                                           tree a function of the pedigree and the options, never of the launch    */
  int32_t shrink_on_failed_contraction; /* 0 = argmin 0.8.1 behaviour; 1 = textbook Nelder-Mead        */
  int32_t max_iters_start;              /* 10000, src/ab_neutral.rs:62                                 */
  int32_t max_iters_boot;               /* 1000,  src/boot_model.rs:81                                 */
  int32_t stream_mode;                  /* pedigrees too large for LDS: 0 = stream the bootstrap observations
                                           (gathered once per fit, 8 B/row/evaluation); 1 = re-stream the u32
                                           index row and gather residuals every evaluation (4 B/row + gather) */
  double sd_tolerance;                  /* f64::EPSILON (argmin default, never overridden)             */
  int32_t window_groups;                /* abn_plan_run: windows are cut into this many groups that run
                                           A -> select -> B concurrently on separate HIP streams
                                           (0 or 1 = one stream, the default; at most 4 overlap: HIP maps
                                           streams onto 4 in-order hardware queues.  Measured gain on a
                                           25-window shard: 2 %, the slowest start chain sets the time)                    */
  int32_t no_fixed_point_skip;          /* 0 (default): a fit whose contraction is rejected has reached a fixed
                                           point of argmin 0.8.1's iteration (the simplex is left untouched and
                                           the cost is deterministic), so it is finished at once with the counters
                                           the repetitions would have produced (iters = max_iters, evals += 2 per
                                           remaining iteration, ABN_FIT_MAX_ITERS): identical outputs.  1 = execute
                                           the repetitions like the reference does                             */
} abn_options;

typedef struct abn_fit_info {
  double best_cost; /* argmin state.best_cost (includes the equilibrium penalty)                        */
  int32_t iters;    /* next_iter() calls                                                                */
  int32_t evals;    /* cost() calls                                                                     */
  int32_t status;   /* ABN_FIT_*                                                                        */
  int32_t lanes;    /* residual reduction tree (accumulators; | rows-per-block code << 8 in stream mode) */
} abn_fit_info;

/* ------------------------------------------------------------------ context */
void abn_default_options(abn_options* opts);
int abn_device_count(int* count);
/* stream == NULL: the context creates (and owns) its own non-blocking HIP stream; ABN_STREAM_DEFAULT: the
 * device's default (null) stream — what torch.cuda.current_stream() is unless the caller switched streams;
 * otherwise the given hipStream_t is borrowed (e.g. torch.cuda.current_stream().cuda_stream != 0). */
#define ABN_STREAM_DEFAULT ((void*)(intptr_t)-1)
int abn_init(int device_ordinal, void* stream, abn_ctx** ctx);
/* Frees the context and its device-buffer pool (the per-call entry points recycle their device buffers through it
 * instead of hipMalloc / hipFree per call).  Destroy the context's plans first. */
int abn_shutdown(abn_ctx* ctx);
/* What abn_init read from hipDeviceProp and the launch geometry derived from it: out4 = {compute units, KiB of LDS per
 * CU, wavefronts of a persistent fit launch, wavefronts of a persistent launch that just about fills the GPU}.  MI355X:
 * {256, 160, 3072, 2048}.  abn_init refuses (ABN_ERR_NO_DEVICE) a device that is not gfx950 or has less LDS per CU.
 * (The reference has no counterpart: rayon sizes its pool from the host's cores, src/ab_neutral.rs:37, src/boot_model.rs:41.) */
int abn_device_info(const abn_ctx* ctx, int32_t* out4);
const char* abn_last_error(const abn_ctx* ctx);
const char* abn_status_string(int status);
int abn_version(void);

/* The residual reduction tree the fits of this pedigree use (what abn_fit_info.lanes reports): a function of the
 * pedigree's generations (N x 3) and opts->lanes_per_chain only — host arithmetic, no device needed. */
int abn_reduction_tree(const abn_options* opts, const double* generations, int32_t n_rows, int32_t* tree);

/* ------------------------------------------------------------------ (1) cost function
 * Replaces `Problem::cost` (src/structs.rs:194-216) + `divergence()` (src/divergence.rs:33-94) for M
 * candidates at once.  pedigree: N x 4 rows (t0,t1,t2,D) exactly as `Pedigree` (src/pedigree.rs:44-45).
 * Observed divergences: column 3 of the pedigree, or, when idx != NULL, the residual bootstrap
 * D*_i = pred[i] + resid[idx[cand_to_boot[m]*N + i]] (src/boot_model.rs:50-57).
 * Outputs: cost[M]; optional dt1t2[M x N] and p_uu_inf[M] (struct Divergence, src/divergence.rs:10-14). */
int abn_cost_batch(abn_ctx* ctx, const abn_options* opts, const double* pedigree, int32_t n_rows,
                   double p_uu0, double eqp, double eqp_weight, const double* candidates, int64_t m,
                   const double* pred, const double* resid, const uint32_t* idx,
                   const uint32_t* cand_to_boot, int64_t n_boot_rows, double* cost, double* dt1t2,
                   double* p_uu_inf);

/* ------------------------------------------------------------------ Nelder-Mead fits
 * Replaces `Executor::new(problem, NelderMead::new(simplex)).max_iters(k).run()` (src/ab_neutral.rs:49-64,
 * src/boot_model.rs:69-84) for F independent fits, one per simplex0[f] (5 vertices x 4).
 * dobs_rows: NULL (every fit uses pedigree column 3) or F x N observed divergences.
 * Outputs in fit order: best[F x 4] (argmin best_param), info[F]. */
int abn_fit_batch(abn_ctx* ctx, const abn_options* opts, const double* pedigree, int32_t n_rows,
                  double p_uu0, double eqp, double eqp_weight, const double* simplex0, int64_t f,
                  const double* dobs_rows, int32_t max_iters, double* best, abn_fit_info* info);
/* The same fits on the sweep kernel (abn_plan_set_stream_sweep): one pass over the rows per Nelder-Mead iteration.  Same
 * outputs, bit for bit.  passes (nullable): passes over the rows, summed over the fits.  ABN_ERR_INVALID_ARG when the
 * pedigree and the options do not route to that kernel (an LDS-resident pedigree, strict order, fewer than 64 lanes per
 * chain, or a footprint beyond the LDS of a CU). */
int abn_fit_batch_sweep(abn_ctx* ctx, const abn_options* opts, const double* pedigree, int32_t n_rows,
                        double p_uu0, double eqp, double eqp_weight, const double* simplex0, int64_t f,
                        const double* dobs_rows, int32_t max_iters, double* best, abn_fit_info* info, int64_t* passes);

/* ------------------------------------------------------------------ deterministic inputs
 * Model::new x5 per start (src/structs.rs:78-96): simplex0[S x 5 x 4] for `window`. Host arithmetic. */
int abn_gen_start_simplices(uint64_t seed, uint32_t window, int32_t n_starts, double max_divergence,
                            double* simplex0);
/* [params, vary() x4] (src/boot_model.rs:69-75, src/structs.rs:100-128) for boots [b0, b0+nb) */
int abn_gen_boot_simplices(uint64_t seed, uint32_t window, uint32_t b0, int64_t nb,
                           const double params[4], double* simplex0);
/* residual-bootstrap indices (src/boot_model.rs:43-48) idx[nb x N], generated ON DEVICE, copied back */
int abn_gen_boot_indices(abn_ctx* ctx, uint64_t seed, uint32_t window, uint32_t b0, int64_t nb,
                         int32_t n_rows, uint32_t* idx);

/* ------------------------------------------------------------------ (2) ab_neutral::run
 * src/ab_neutral.rs:13-142: n_starts random-start fits (start simplices from opts->seed), arg-min by
 * pure LSE (:83-101), predicted divergence (:123-129) and residuals (:131-135).
 * Outputs: model[4], pred[N], resid[N]; optional all_models[S x 4], info[S], lse[S]. */
int abn_ab_neutral_run(abn_ctx* ctx, const abn_options* opts, const double* pedigree, int32_t n_rows,
                       double p0uu, double eqp, double eqp_weight, int32_t n_starts, double* model,
                       double* pred, double* resid, double* all_models, abn_fit_info* info,
                       double* lse);

/* src/ab_neutral.rs:83-135 on its own: stable arg-min by pure LSE (serial row order, no penalty term) over
 * S fitted models, then predicted divergence and residuals of the winner.  NaN never wins; *best_index = -1
 * (and ABN_ERR_NO_FINITE_FIT) if every LSE is NaN.  lse[S] optional. */
int abn_select_best(abn_ctx* ctx, const double* pedigree, int32_t n_rows, double p0uu, const double* models,
                    int32_t n_models, int32_t* best_index, double* model, double* pred, double* resid,
                    double* lse);

/* src/boot_model.rs:86-91 on its own: raw[B x 7] = [alpha, beta, weight, intercept, est_mm, est_um, est_uu]
 * (src/structs.rs:146-159) from fitted vectors best[B x 4], evaluated on the device. */
int abn_bootstrap_rows(abn_ctx* ctx, const double* best, int64_t n_boot, double* raw);

/* ------------------------------------------------------------------ (3) boot_model::run
 * src/boot_model.rs:17-115 without the PNG (:105-109): n_boot residual-bootstrap refits.
 * raw[n_boot x 7] = [alpha,beta,weight,intercept,PrMM,PrUM,PrUU] rows (RawAnalysis, src/analysis.rs:12),
 * row b = bootstrap b (the reference's row order is thread-schedule dependent).  info optional. */
int abn_boot_model_run(abn_ctx* ctx, const abn_options* opts, const double* pedigree, int32_t n_rows,
                       const double* model, const double* pred, const double* resid, double p0uu,
                       double eqp, double eqp_weight, int32_t n_boot, double* raw,
                       abn_fit_info* info);

/* src/analysis.rs:50-98 on the host: out[32] = mean[8], sd[8], ci_lo[8], ci_hi[8] in the order
 * alpha, beta, beta/alpha, weight, intercept, pr_mm, pr_um, pr_uu (struct Analysis, :15-47).
 * A table with a NaN in raw or in beta/alpha (rows of fits with status ABN_FIT_NONFINITE) is refused with
 * ABN_ERR_NO_FINITE_FIT and out32 is not written: the quantiles sort with `<` (the reference converts to n64, which
 * rejects NaN, :57-58).  +-inf is not refused.  The host mirrors (RawAnalysis::analyze, the Python analyze()) make the
 * same test first, for a message that names the bootstrap. */
int abn_analyze(const double* raw, int64_t n_boot, double* out32);

/* ------------------------------------------------------------------ the analysis on the device, all windows at once
 * src/analysis.rs:50-98 for every window of a bootstrap table in one launch: raw[n_windows x n_boot x 7] (window w's
 * table as abn_analyze takes it) -> out[n_windows x 32], window w in abn_analyze's layout, every number bit-identical
 * to abn_analyze on that window's table; first_bad[n_windows] (int32, may be NULL) = the smallest bootstrap index whose
 * row holds a NaN or whose beta/alpha is NaN (the test of abn_analyze; +-inf is not refused), -1 if there is none.  A
 * window with first_bad >= 0 gets 32 NaN; the other windows are unaffected.  n_boot = 1: sd is NaN, as on the host.
 * ABN_ERR_INVALID_ARG: null raw or out, n_windows < 0, n_boot <= 0 or above 2^31 - 1.  n_windows == 0: ABN_OK, nothing
 * is written.  ABN_ERR_NO_FINITE_FIT — AFTER filling every buffer — when any window has first_bad >= 0 (the
 * convention of abn_plan_download).  raw, out and first_bad are HOST arrays here. */
int abn_analyze_batch(abn_ctx* ctx, const double* raw, int32_t n_windows, int64_t n_boot, double* out,
                      int32_t* first_bad);
/* src/analysis.rs:50-98 as above on DEVICE-resident buffers (no table crosses PCIe): dev_raw f64[n_windows x n_boot x 7],
 * dev_out f64[n_windows x 32], dev_first_bad i32[n_windows] (may be NULL).  kernel_ms (nullable): HIP-event time of the
 * kernel on the context's stream.  Returns after the work has completed, with the statuses above. */
int abn_analyze_batch_dev(abn_ctx* ctx, const void* dev_raw, int32_t n_windows, int64_t n_boot, void* dev_out,
                          void* dev_first_bad, double* kernel_ms);

/* ------------------------------------------------------------------ pedigree construction
 * DMatrix::from (src/pedigree.rs:210-261): pairwise divergence of n samples over n_sites aligned sites.
 *   codes[n x n_sites] (u8, row per sample): status_numeric 0 = U, 1 = I, 2 = M
 *   (src/methylation_site.rs:130-136), plus 0x80 when the site's posteriormax is below the filter (the
 *   site is then skipped for every pair it takes part in, src/pedigree.rs:249-251).
 * Outputs per unordered pair i < j at index p = i*n - i*(i+1)/2 + (j - i - 1) (the nested-loop order of
 * :214-215):  diff[p] = sum of |status_i - status_j| over sites valid in both (:253),  both[p] = number of
 * such sites (:254),  dvalue[p] = diff / (2 * both) in f64 (:257; NaN for both == 0 like the reference's
 * 0/0).  Integer sums are exact, so the result does not depend on the device's summation order.
 * Any number of samples up to 65535 (the reference has no limit; the sample axis is tiled in groups of 64), any
 * number of sites, codes at any byte alignment.  Bytes other than 0, 1, 2 (| 0x80) are not valid codes. */
int abn_pairwise_divergence(abn_ctx* ctx, const uint8_t* codes, int32_t n_samples, int64_t n_sites,
                            uint64_t* diff, uint64_t* both, double* dvalue);
/* The same on DEVICE-resident buffers (no PCIe in the call): dev_codes u8[n x n_sites]; dev_diff / dev_both
 * u64[pairs], dev_dvalue f64[pairs], any of the three may be NULL.  kernel_ms (nullable): HIP-event time of the
 * kernels of this call on the context's stream.  Returns after the work has completed. */
int abn_pairwise_divergence_dev(abn_ctx* ctx, const void* dev_codes, int32_t n_samples, int64_t n_sites,
                                void* dev_diff, void* dev_both, void* dev_dvalue, double* kernel_ms);
/* The same for MANY column ranges ("windows") of one code matrix in one batched call — the window loop of
 * src/cli/metaprofile.rs:50-72 around DMatrix::from (src/pedigree.rs:210-261): codes[n_samples x row_stride], window w =
 * the sites [site_begin[w], site_end[w]) of every sample's row.  Windows may overlap, leave gaps, be empty and begin or
 * end at any byte; site_begin / site_end are HOST arrays of n_windows entries.  Outputs are [n_windows x pairs], window
 * w's block in the pair order above; every value is bit-identical to abn_pairwise_divergence on that window's columns
 * (an empty or wholly filtered window: both = 0, dvalue = NaN).  Any output may be NULL.  The number of kernel launches
 * does not depend on n_windows (short windows are one launch in all; see DESIGN.md §4 "Pairwise").
 * ABN_ERR_INVALID_ARG: null codes, n_windows < 0, a window with begin < 0, begin > end or end > row_stride,
 * n_samples > 65535.  n_windows == 0 or n_samples < 2: ABN_OK, nothing is written. */
int abn_pairwise_divergence_windows(abn_ctx* ctx, const uint8_t* codes, int32_t n_samples, int64_t row_stride,
                                    const int64_t* site_begin, const int64_t* site_end, int32_t n_windows,
                                    uint64_t* diff, uint64_t* both, double* dvalue);
/* ... and on DEVICE-resident codes and outputs (src/pedigree.rs:210-261, src/cli/metaprofile.rs:50-72): dev_codes
 * u8[n_samples x row_stride] at any byte alignment; dev_diff / dev_both u64[n_windows x pairs], dev_dvalue
 * f64[n_windows x pairs], any may be NULL; kernel_ms as above.  Returns after the work has completed. */
int abn_pairwise_divergence_windows_dev(abn_ctx* ctx, const void* dev_codes, int32_t n_samples, int64_t row_stride,
                                        const int64_t* site_begin, const int64_t* site_end, int32_t n_windows,
                                        void* dev_diff, void* dev_both, void* dev_dvalue, double* kernel_ms);

/* ------------------------------------------------------------------ 2-bit packed codes for the scan above
 * DMatrix::from (src/pedigree.rs:210-261) reads two bits of every code byte: U, I, M, or "filtered for this sample".
 * The packed format stores just those — a quarter of the bytes to keep, to upload and to read:
 *   one 2-bit field per (sample, site): 0 = U, 1 = I, 2 = M (status_numeric, src/methylation_site.rs:130-136),
 *   3 = filtered (posteriormax below the filter, src/pedigree.rs:249-251);
 *   sites in groups of 16, one little-endian dword per group: site 16 g + 4 j + e (j, e in 0..3) is stored in byte e of
 *   dword g at bits 2j..2j+1 — so (dword >> 2j) & 0x03030303 is four byte-sized codes;
 *   sample i's row starts at packed + i * row_stride_bytes; row_stride_bytes is a multiple of 64 (256 sites), at least
 *   abn_packed_row_stride(n_sites); EVERY field from site n_sites to the end of the row must be 3 (the scan does not
 *   check it; abn_pack_codes writes it); a device-resident buffer is 16-byte aligned (a host buffer: any alignment).
 * Both forms of the scan take packed codes: one whole matrix (abn_pairwise_divergence_packed*) and many column ranges
 * of one matrix in one call (abn_pairwise_divergence_windows_packed*, below).  A window may begin and end at any site:
 * the scan reads whole 64-byte steps of the rows and treats the fields outside the window as filtered.
 *
 * Host arithmetic, no device: bytes per row for n_sites sites — ceil(n_sites / 256) * 64; 0 for n_sites <= 0. */
int64_t abn_packed_row_stride(int64_t n_sites);
/* src/pedigree.rs:210-261, the codes of abn_pairwise_divergence -> packed rows (host arithmetic, no device).
 * codes[n_samples rows of src_row_stride bytes, the first n_sites used]; packed[n_samples x row_stride_bytes], padding
 * fields included, is written.  ABN_ERR_INVALID_ARG: a null pointer, a negative size, src_row_stride < n_sites, a
 * row_stride_bytes that is not a multiple of 64 or is below abn_packed_row_stride(n_sites), or a byte that is not 0, 1, 2
 * or 0x80 | anything (the contents of packed are then unspecified). */
int abn_pack_codes(const uint8_t* codes, int32_t n_samples, int64_t n_sites, int64_t src_row_stride, uint8_t* packed,
                   int64_t row_stride_bytes);
/* ... and back (src/pedigree.rs:210-261): codes[n_samples rows of dst_row_stride bytes] receive 0, 1, 2, or 0x80 for a
 * filtered site (the status under the flag is not kept).  Same argument rules. */
int abn_unpack_codes(const uint8_t* packed, int32_t n_samples, int64_t n_sites, int64_t row_stride_bytes, uint8_t* codes,
                     int64_t dst_row_stride);
/* abn_pairwise_divergence (src/pedigree.rs:210-261) on packed codes: the same outputs, bit for bit, in the same pair
 * order, with the same NULL rules.  ABN_ERR_INVALID_ARG: null packed, n_samples <= 0 or > 65535, n_sites < 0, a
 * row_stride_bytes that is not a multiple of 64 or is below abn_packed_row_stride(n_sites).  n_samples < 2: ABN_OK,
 * nothing is written.  n_sites == 0: both = diff = 0, dvalue = NaN. */
int abn_pairwise_divergence_packed(abn_ctx* ctx, const uint8_t* packed, int32_t n_samples, int64_t n_sites,
                                   int64_t row_stride_bytes, uint64_t* diff, uint64_t* both, double* dvalue);
/* ... and on DEVICE-resident packed codes and outputs (src/pedigree.rs:210-261), as abn_pairwise_divergence_dev:
 * dev_packed u8[n_samples x row_stride_bytes], 16-byte aligned (else ABN_ERR_INVALID_ARG); any output may be NULL;
 * kernel_ms as above.  Returns after the work has completed. */
int abn_pairwise_divergence_packed_dev(abn_ctx* ctx, const void* dev_packed, int32_t n_samples, int64_t n_sites,
                                       int64_t row_stride_bytes, void* dev_diff, void* dev_both, void* dev_dvalue,
                                       double* kernel_ms);

/* abn_pairwise_divergence_windows (the window loop of src/cli/metaprofile.rs:50-72 around DMatrix::from,
 * src/pedigree.rs:210-261) on packed codes: packed[n_samples x row_stride_bytes] holds n_sites sites per row in the
 * format above; window w = the sites [site_begin[w], site_end[w]) of every row, HOST arrays of n_windows entries, in
 * sites.  Windows may overlap, leave gaps, be empty and begin or end at any site.  Outputs are [n_windows x pairs] in the
 * order, with the NULL rules and with the bits of abn_pairwise_divergence_windows on the unpacked codes (an empty or
 * wholly filtered window: diff = both = 0, dvalue = NaN).
 * ABN_ERR_INVALID_ARG: what abn_pairwise_divergence_packed refuses (null packed, n_samples <= 0 or > 65535, n_sites < 0,
 * a row_stride_bytes that is not a multiple of 64 or is below abn_packed_row_stride(n_sites)); n_windows < 0; null window
 * arrays with n_windows > 0; a window with begin < 0, begin > end or end > n_sites; a window so long that
 * a chunk of it (a job of the scan) would reach 2^30 sites.  n_windows == 0 or n_samples < 2: ABN_OK, nothing is written. */
int abn_pairwise_divergence_windows_packed(abn_ctx* ctx, const uint8_t* packed, int32_t n_samples, int64_t n_sites,
                                           int64_t row_stride_bytes, const int64_t* site_begin, const int64_t* site_end,
                                           int32_t n_windows, uint64_t* diff, uint64_t* both, double* dvalue);
/* ... and on DEVICE-resident packed codes and outputs (src/cli/metaprofile.rs:50-72, src/pedigree.rs:210-261):
 * dev_packed u8[n_samples x row_stride_bytes], 16-byte aligned (else ABN_ERR_INVALID_ARG); dev_diff / dev_both
 * u64[n_windows x pairs], dev_dvalue f64[n_windows x pairs], any may be NULL; site_begin / site_end stay HOST arrays;
 * kernel_ms as above.  Returns after the work has completed. */
int abn_pairwise_divergence_windows_packed_dev(abn_ctx* ctx, const void* dev_packed, int32_t n_samples, int64_t n_sites,
                                               int64_t row_stride_bytes, const int64_t* site_begin,
                                               const int64_t* site_end, int32_t n_windows, void* dev_diff,
                                               void* dev_both, void* dev_dvalue, double* kernel_ms);

/* The 3 x 3 state transitions of every pair — the joint table behind src/pedigree.rs:236-257, of which `both` and `diff`
 * are two folds: table[p][3 x + y] = the sites both samples of pair p = (a, b), a < b, keep with status x in sample a and
 * y in sample b (0 = U, 1 = I, 2 = M), so that both = sum of the nine and diff = sum of |x - y| table[p][3 x + y]; entries 2
 * (U -> M) and 6 (M -> U) are the observed gains and losses between a and b.  table: uint64 [pairs x 9] in the pair order
 * above, exact.  Arguments and refusals as abn_pairwise_divergence_packed (nothing is read or written before one); a NULL
 * table with n_samples >= 2: ABN_ERR_INVALID_ARG.  n_samples < 2: ABN_OK, nothing is written.  n_sites = 0: all zero. */
int abn_pairwise_transitions_packed(abn_ctx* ctx, const uint8_t* packed, int32_t n_samples, int64_t n_sites,
                                    int64_t row_stride_bytes, uint64_t* table);
/* ... on DEVICE-resident packed codes and table: dev_packed 16-byte aligned (else ABN_ERR_INVALID_ARG), dev_table
 * u64[pairs x 9]; kernel_ms as above.  Returns after the work has completed. */
int abn_pairwise_transitions_packed_dev(abn_ctx* ctx, const void* dev_packed, int32_t n_samples, int64_t n_sites,
                                        int64_t row_stride_bytes, void* dev_table, double* kernel_ms);
/* ... and of many windows of one packed matrix in one batch (src/cli/metaprofile.rs:50-72): table uint64
 * [n_windows x pairs x 9], window w's block equal to abn_pairwise_transitions_packed on that window's columns (an empty or
 * wholly filtered window: all zero).  Arguments and refusals as abn_pairwise_divergence_windows_packed and its _dev form.
 * n_windows == 0 or n_samples < 2: ABN_OK, nothing is written. */
int abn_pairwise_transitions_windows_packed(abn_ctx* ctx, const uint8_t* packed, int32_t n_samples, int64_t n_sites,
                                            int64_t row_stride_bytes, const int64_t* site_begin, const int64_t* site_end,
                                            int32_t n_windows, uint64_t* table);
int abn_pairwise_transitions_windows_packed_dev(abn_ctx* ctx, const void* dev_packed, int32_t n_samples, int64_t n_sites,
                                                int64_t row_stride_bytes, const int64_t* site_begin,
                                                const int64_t* site_end, int32_t n_windows, void* dev_table,
                                                double* kernel_ms);
/* The state census of a packed matrix per column range: counts uint64 [n_windows x n_samples x 3], the fields 0, 1 and 2
 * (U, I, M of src/pedigree.rs:253-257) that each sample holds inside [site_begin[w], site_end[w]) — what rc_meth_lvl over a
 * sample's OWN kept sites needs (src/pedigree.rs:159-175; the pair tables above count only the sites both samples of a pair
 * keep).  Exact integers, summed without atomics; an empty window gives zeros.  Arguments and refusals are those of
 * abn_pairwise_divergence_windows_packed(_dev), but one sample is served.  HOST matrix and counts. */
int abn_packed_census_windows(abn_ctx* ctx, const uint8_t* packed, int32_t n_samples, int64_t n_sites,
                              int64_t row_stride_bytes, const int64_t* site_begin, const int64_t* site_end,
                              int32_t n_windows, uint64_t* counts);
/* ... DEVICE matrix (16-byte aligned) and DEVICE counts, HOST window arrays; kernel_ms (may be NULL): the HIP-event time of
 * the two kernels.  Returns after the work has completed. */
int abn_packed_census_windows_dev(abn_ctx* ctx, const void* dev_packed, int32_t n_samples, int64_t n_sites,
                                  int64_t row_stride_bytes, const int64_t* site_begin, const int64_t* site_end,
                                  int32_t n_windows, void* dev_counts, double* kernel_ms);
/* Region-level states: one field per (sample, region), called from the sample's single-site fields inside the region and
 * written in the packed format above, so that every packed scan and the census take the result as a matrix of sites.
 * THE LAW.  Inputs: packed[n_samples x row_stride_bytes] of n_sites sites (format above); T = n_windows windows
 * [site_begin[t], site_end[t]), any column ranges of the rows, overlapping or empty; a column map src[C], C = n_columns,
 * src[c] in [0, T), repeats and omissions allowed (NULL: the identity, and C must be T); a rule of exact integers with
 * 0 <= lo_num <= hi_num <= den, 1 <= den <= 2^20, min_kept >= 1.  For sample s and window t let n0, n1, n2 be the fields
 * 0, 1, 2 of row s inside the window (what abn_packed_census_windows counts), kept = n0 + n1 + n2, m = n1 + 2 n2 (twice the
 * sum of state / 2, the level abn_sim_pedigree and abn_sim_study use).  The region's field is 3 if kept < min_kept (an
 * empty window is always 3); 0 if m den < lo_num 2 kept; 2 if m den > hi_num 2 kept; 1 otherwise (equality on either side
 * is 1).  64-bit unsigned arithmetic: n_sites <= 2^34 and den <= 2^20 keep both products below 2^56; no floating point.
 * Output: out_packed[n_samples x abn_packed_row_stride(C)], column c of row s the field of window src[c], the fields from
 * C to the end of the stride 3.  One fused kernel counts, calls and packs (one lane per output field); windows of at least
 * long_sites sites (0: the library's default; else a multiple of 16, at most 2^29) are counted by the census kernels first.
 * ABN_ERR_INVALID_ARG with a text, before any launch: what abn_packed_census_windows refuses; a rule outside the bounds;
 * src[c] outside [0, T) (the text names the column); src NULL with n_columns != n_windows; n_windows or n_columns above
 * INT32_MAX; long_sites negative or no multiple of 16.  n_columns == 0: ABN_OK, nothing is written.  HOST buffers. */
int abn_packed_region_states(abn_ctx* ctx, const uint8_t* packed, int32_t n_samples, int64_t n_sites,
                             int64_t row_stride_bytes, const int64_t* site_begin, const int64_t* site_end, int64_t n_windows,
                             const int32_t* src, int64_t n_columns, int64_t lo_num, int64_t hi_num, int64_t den,
                             int64_t min_kept, int64_t long_sites, uint8_t* out_packed);
/* ... DEVICE matrix (16-byte aligned) and DEVICE output, HOST window and src arrays; ms2 (may be NULL): the HIP-event times
 * of the long windows' census and of the kernel.  Returns after the work has completed. */
int abn_packed_region_states_dev(abn_ctx* ctx, const void* dev_packed, int32_t n_samples, int64_t n_sites,
                                 int64_t row_stride_bytes, const int64_t* site_begin, const int64_t* site_end,
                                 int64_t n_windows, const int32_t* src, int64_t n_columns, int64_t lo_num, int64_t hi_num,
                                 int64_t den, int64_t min_kept, int64_t long_sites, void* dev_out, double* ms2);

/* ------------------------------------------------------------------ window placement (the `extract` stage)
 * Windows::extract (src/windows.rs:287-343) behind the gene choice: MethylationSite::place_in_windows
 * (src/methylation_site.rs:423-490) for every site of every sample, on the device, straight into the packed matrix
 * abn_pairwise_divergence_windows_packed* scans — no <region>/<window>/<sample> file tree (Windows::save,
 * src/windows.rs:259-285) in between.  The gene of every site (find_gene with the last_gene cache, :303-338) is chosen on
 * the host for abn_windows_create, which takes its result, and on the device for abn_windows_create_sites (abn_genes_*
 * below).  Global window index: upstream 0.., then gene, then downstream. */
typedef struct abn_windows abn_windows;
typedef struct abn_windows_params {
  uint32_t cutoff;       /* arguments::Windows (src/arguments.rs:6-62)                                          */
  uint32_t step;         /* window_step after the 0 -> window_size default (src/extract.rs:26-28); not 0        */
  uint32_t size;         /* window_size                                                                         */
  int32_t absolute;
  int32_t n_upstream;    /* Windows::new (src/windows.rs:28-44): cutoff / step, or 100 / step when not absolute */
  int32_t n_gene;        /* max_gene_length / step, or 100 / step                                               */
  int32_t n_downstream;  /* as n_upstream                                                                       */
} abn_windows_params;
/* Replaces the loop of Windows::extract (src/windows.rs:325-339) from place_in_windows on, and Windows::save
 * (:259-285), for n_samples methylomes.  Struct-of-arrays over all samples, concatenated in file order: sample s owns the
 * sites [site_offset[s], site_offset[s + 1]) (site_offset[0] = 0; under 2^32 sites per sample).  Per site: pos = start
 * (src/methylation_site.rs:431); gene_start / gene_end of its gene; flags bit 0 = the site is on the antisense strand
 * (Unknown counts as sense, :439-443), bit 1 = it has a gene (without: the site is in no window); code = status | 0x80
 * when the posterior is below the filter (the byte of abn_pairwise_divergence); level = meth_lvl.
 * Uploads, places, ranks, packs and sums; *out is device-resident until abn_windows_destroy (destroy it before its
 * context).  W = n_upstream + n_gene + n_downstream windows.  A window in which the samples' site counts differ is
 * RAGGED: flagged, and given an empty column range (the reference compares such pairs as D = 0, src/pedigree.rs:210-261).
 * ABN_ERR_INVALID_ARG: null pointers, n_samples <= 0 or > 65535, step 0, negative window counts, a site_offset that is
 * not ascending from 0. */
int abn_windows_create(abn_ctx* ctx, const abn_windows_params* params, int32_t n_samples, const int64_t* site_offset,
                       const uint32_t* pos, const uint32_t* gene_start, const uint32_t* gene_end, const uint8_t* flags,
                       const uint8_t* code, const double* level, abn_windows** out);
int abn_windows_destroy(abn_windows* h);
/* the matrix Windows::save's files (src/windows.rs:259-285) would have been packed into: W, bytes per row, fields per row
 * (4 x row_stride: the n_sites of abn_pairwise_divergence_windows_packed); any pointer may be NULL */
int abn_windows_info(const abn_windows* h, int32_t* n_windows, int64_t* row_stride, int64_t* n_sites);
/* [n_samples x W] each, any may be NULL: count = Windows::distribution (src/windows.rs:158-165); level_sum = the fold of
 * Windows::steady_state_methylation before its division (:94-128), in push order; level_sum_kept / kept = sum and number
 * of the levels whose posterior passes the filter (src/pedigree.rs:165-166), in push order */
int abn_windows_stats(const abn_windows* h, int64_t* count, double* level_sum, double* level_sum_kept, int64_t* kept);
/* [W] each, any may be NULL: window w's sites are the fields [begin[w], end[w]) of every row (begin a multiple of 256), in
 * the order Windows::extract pushed them (src/windows.rs:335); ragged[w] = 1: the counts differ, begin[w] == end[w] */
int abn_windows_layout(const abn_windows* h, int64_t* begin, int64_t* end, int32_t* ragged);
/* the packed matrix [n_samples x row_stride] (format above; what layout_packed_call of the host layer writes from the
 * files of src/windows.rs:259-285): copied to the host, or its device pointer (16-byte aligned, owned by the handle) */
int abn_windows_packed(abn_windows* h, uint8_t* host_out);
int abn_windows_packed_device_ptr(abn_windows* h, void** dev_ptr);
/* DMatrix::from (src/pedigree.rs:210-261) of every window (the loop of src/cli/metaprofile.rs:50-72):
 * abn_pairwise_divergence_windows_packed_dev on the resident matrix with the handle's begin / end.  HOST outputs
 * [W x pairs], any may be NULL; a ragged or empty window: diff = both = 0, dvalue = NaN.  n_samples < 2: nothing written. */
int abn_windows_pairwise(abn_windows* h, uint64_t* diff, uint64_t* both, double* dvalue);

/* ------------------------------------------------------------------ the gene of every site (the `extract` stage)
 * The loop of Windows::extract (src/windows.rs:325-338) up to place_in_windows: a site keeps the previous site's gene
 * while is_in_gene holds (src/methylation_site.rs:368-378), else find_gene (:385-418: slice::binary_search_by over the
 * list of the site's chromosome and strand, probe for probe, then is_in_gene).  The last_gene cache is resolved on the
 * device without iteration: per block of 1024 sites every site's find_gene and its chain of misses, one pass per sample
 * over its blocks for the gene carried into each, then every site's gene (csrc/abn_genes.hpp).  Results equal the serial
 * loop's, element for element. */
typedef struct abn_genes abn_genes;
typedef struct abn_gene_rule {  /* the two arguments is_in_gene and find_gene read (src/arguments.rs:6-62) */
  uint32_t cutoff;
  int32_t cutoff_gene_length;   /* not 0: a gene's own length is its cutoff */
} abn_gene_rule;
/* The annotation as src/extract.rs:30-67 holds it, device-resident until abn_genes_destroy (destroy it before its
 * context): n_lists lists, list l = the genes [list_offset[l], list_offset[l + 1]) of gene_start / gene_end / gene_strand
 * (0 Sense, 1 Antisense, 2 Unknown), belonging to chromosome list_chromosome[l] (Numbered(n) = n, Mitochondrial = 256,
 * Chloroplast = 257) and kind list_kind[l] (0 sense, 1 antisense, 2 combined: the three lists of GenesByStrand,
 * src/genes.rs:127-163).  Every list is as :61-66 leaves it, stably sorted by start; the library does not sort.
 * ABN_ERR_INVALID_ARG: null pointers, n_lists < 0, a chromosome outside 0..257, a kind outside 0..2, a (chromosome, kind)
 * given twice, a gene_strand above 2, list_offset not ascending from 0 (or beyond 2^32 - 2 genes). */
int abn_genes_create(abn_ctx* ctx, int32_t n_lists, const int32_t* list_chromosome, const int32_t* list_kind,
                     const int64_t* list_offset, const uint32_t* gene_start, const uint32_t* gene_end,
                     const uint8_t* gene_strand, abn_genes** out);
int abn_genes_destroy(abn_genes* h);
/* Replaces the loop of Windows::extract (src/windows.rs:325-338) in front of place_in_windows, with is_in_gene and
 * find_gene (src/methylation_site.rs:368-418), for n_samples methylomes.  Struct-of-arrays over all samples as in
 * abn_windows_create (site_offset, HOST memory in both forms); per site the fields of abn_sites_fetch: chromosome, start,
 * end, strand.  Outputs per site, the arrays abn_windows_create takes: gene_start, gene_end (0, 0 without a gene), flags
 * (bit 0: antisense site, bit 1: has a gene).  The cache starts empty at every sample's first site.  kernel_ms (may be
 * NULL): double[3], the HIP-event times of the three kernels.  Zero sites, or a sample of zero sites, is fine.
 * ABN_ERR_INVALID_ARG: null pointers, n_samples <= 0 or > 65535, site_offset not ascending from 0, a site chromosome
 * outside 0..257 or a strand above 2 (host form: nothing is launched; device form: found by the kernels, the outputs are
 * then unspecified). */
int abn_genes_choose(abn_genes* h, const abn_gene_rule* rule, int32_t n_samples, const int64_t* site_offset,
                     const int32_t* chromosome, const uint32_t* start, const uint32_t* end, const uint8_t* strand,
                     uint32_t* gene_start, uint32_t* gene_end, uint8_t* flags, double* kernel_ms);
/* ... on DEVICE-resident site arrays and outputs; returns after the work has completed */
int abn_genes_choose_dev(abn_genes* h, const abn_gene_rule* rule, int32_t n_samples, const int64_t* site_offset,
                         const void* dev_chromosome, const void* dev_start, const void* dev_end, const void* dev_strand,
                         void* dev_gene_start, void* dev_gene_end, void* dev_flags, double* kernel_ms);
/* abn_windows_create behind abn_genes_choose_dev, nothing coming back in between (src/windows.rs:325-339 whole): the
 * site fields are uploaded once, the genes chosen on the device and pos = start, gene_start, gene_end, flags handed to
 * the placement as device arrays.  code and level as in abn_windows_create.  *out is an ordinary abn_windows.
 * ABN_ERR_INVALID_ARG: as abn_windows_create and abn_genes_choose, and a `genes` of another context. */
int abn_windows_create_sites(abn_ctx* ctx, const abn_windows_params* params, abn_genes* genes, const abn_gene_rule* rule,
                             int32_t n_samples, const int64_t* site_offset, const int32_t* chromosome,
                             const uint32_t* start, const uint32_t* end, const uint8_t* strand, const uint8_t* code,
                             const double* level, abn_windows** out);

/* ------------------------------------------------------------------ methylome text -> site records
 * MethylationSite::from_methylome_file_line (src/methylation_site.rs:146-362, without --invert) for every line of a
 * methylome file's text, on the device: a line index (the '\n' bytes, BufRead::lines), a lane per line parsing from LDS,
 * a stable compaction.  Lines are numbered from 0 in the file (the header row is line 0).  A line is a site, no site, or
 * DEFERRED: the device gives an f64 field (posteriormax, meth_lvl) a value only where one IEEE operation is certain to
 * give str::parse::<f64>'s bits — [sign] digits [.] digits [e [sign] digits], at most 19 significant digits, their
 * integer at most 2^53, a decimal exponent within +-22 — and a line with any other such token that could still be a site
 * (inf, nan, 20 digits, 1e30 ...), or a line longer than 16 KiB, is handed back for the caller to parse on the host. */
typedef struct abn_sites abn_sites;
typedef struct abn_sites_params {
  int64_t slab_bytes;  /* the text is parsed in slabs of at most this many bytes, cut at line ends (a longer line is a
                          slab of its own); bounds the device memory of a call.  0: 64 MiB; at most 1 GiB */
  int32_t skip_lines;  /* leading lines not parsed: 1 for the loop of Windows::extract (`lines.skip(1)`,
                          src/windows.rs:303-306), 0 for that of Pedigree::build (src/pedigree.rs:147-163) */
  int32_t contexts;    /* the methylation contexts whose lines are sites, as a mask: 1 CG, 2 CHG, 4 CHH (field 3 of the
                          9-, 10- and 11-field formats).  0: CG alone, as the reference (src/methylation_site.rs:150,193);
                          the 4-field rows have no context and are sites under every mask */
} abn_sites_params;
/* Replaces the line loops of Windows::extract (src/windows.rs:303-338) and Pedigree::build (src/pedigree.rs:147-163)
 * up to and including from_methylome_file_line (src/methylation_site.rs:146-362).  text: n_bytes bytes of HOST memory
 * (no terminator needed; "\n" or "\r\n" ends a line, a last line without one is a line).  params NULL: slab_bytes 0,
 * skip_lines 1.  The results are on the host when the call returns; *out holds them until abn_sites_destroy.
 * ABN_ERR_INVALID_ARG: null pointers, n_bytes < 0, slab_bytes outside [0, 2^30], skip_lines < 0, contexts outside
 * [0, 7], a line of over 2 GiB. */
int abn_sites_parse(abn_ctx* ctx, const char* text, int64_t n_bytes, const abn_sites_params* params, abn_sites** out);
int abn_sites_destroy(abn_sites* h);
/* the counts behind src/windows.rs:303-338: accepted sites, deferred lines, lines of the text (skipped ones included);
 * kernel_ms = the HIP-event time of the call's kernels, summed over the slabs.  Any pointer may be NULL */
int abn_sites_info(const abn_sites* h, int64_t* n_sites, int64_t* n_deferred, int64_t* n_lines, double* kernel_ms);
/* The accepted sites in file order, [n_sites] each, any may be NULL — the fields of MethylationSite
 * (src/methylation_site.rs:32-45) the extraction and the pedigree build read: line; chromosome (Numbered(n) = n,
 * Mitochondrial = 256, Chloroplast = 257, src/methylation_site.rs:48-68); start, end; strand (0 Sense, 1 Antisense,
 * 2 Unknown); posteriormax; status (U 0, I 1, M 2, src/methylation_site.rs:130-136); status_flag (1: the status byte
 * is none of M, I, U and was parsed as U — the reference prints a warning there, src/methylation_site.rs:107-112);
 * meth_lvl */
int abn_sites_fetch(const abn_sites* h, int64_t* line, int32_t* chromosome, uint32_t* start, uint32_t* end,
                    uint8_t* strand, double* posteriormax, uint8_t* status, uint8_t* status_flag, double* meth_lvl);
/* The deferred lines in file order, [n_deferred] each, any may be NULL: line, the offset of its first byte in text, its
 * length without the line end — to be decided by the host's from_methylome_file_line (src/methylation_site.rs:146-362) */
int abn_sites_deferred(const abn_sites* h, int64_t* line, int64_t* offset, int64_t* length);
/* abn_sites_parse with the records left where the device wrote them (the same lines of src/windows.rs:303-338 and
 * src/methylation_site.rs:146-362; the same text, slabs, skip_lines, kernels and argument checks): every slab's compacted
 * record arrays stay on the device, owned by *out until abn_sites_destroy (destroy it before its context).  What comes
 * back is what the host has to decide or to say: the deferred triples, and the lines of the records whose status_flag is
 * set.  abn_sites_info (n_sites = the device's records plus the inserted ones), abn_sites_deferred and abn_sites_fetch
 * (downloads, and merges the inserted records in by line) work on such a RESIDENT handle as on the host form. */
int abn_sites_parse_dev(abn_ctx* ctx, const char* text, int64_t n_bytes, const abn_sites_params* params, abn_sites** out);
/* The file lines of the accepted records whose status byte was none of M, I, U — where src/methylation_site.rs:107-112
 * prints its warning — ascending; *n their number, line [*n]; either may be NULL.  Both forms. */
int abn_sites_flagged(const abn_sites* h, int64_t* n, int64_t* line);
/* Hands a RESIDENT handle the deferred lines that the host's from_methylome_file_line (src/methylation_site.rs:146-362)
 * accepted — the second branch of the merge by line that the loop of src/windows.rs:303-338 performs implicitly — [n]
 * each, line strictly ascending, every entry one of the handle's deferred lines; status U 0, I 1, M 2.  Uploaded once;
 * nothing is launched.  At most once per handle; n = 0 is fine (no deferred line was a site).
 * ABN_ERR_INVALID_ARG: a host-form handle, a second call, null arrays with n > 0, a line that was not deferred, lines not
 * ascending, a chromosome outside 0..257, a strand or a status above 2. */
int abn_sites_insert(abn_sites* h, int64_t n, const int64_t* line, const int32_t* chromosome, const uint32_t* start,
                     const uint32_t* end, const uint8_t* strand, const double* posteriormax, const uint8_t* status,
                     const double* meth_lvl);
/* ---- methylation contexts: one parse, one resident handle per context
 * A handle parsed with abn_sites_params.contexts keeps every site's CONTEXT CODE — CG 0, CHG 1, CHH 2, and 3 for the
 * 4-field rows, which have none — beside its record (two bits of the device records' meta word).
 * abn_sites_context: *mask = the contexts the handle was parsed under (1 for contexts 0), context [n_sites] = every
 * site's code in the order of abn_sites_fetch; either may be NULL.  Both forms. */
int abn_sites_context(const abn_sites* h, int32_t* mask, uint8_t* context);
/* abn_sites_insert with every record's context code.  abn_sites_insert is this call with every code 0, and is refused
 * (ABN_ERR_INVALID_ARG) with n > 0 on a handle whose mask is not CG alone.
 * ABN_ERR_INVALID_ARG: as abn_sites_insert, and a code above 3 or a code 0..2 outside the handle's mask. */
int abn_sites_insert_ctx(abn_sites* h, int64_t n, const int64_t* line, const int32_t* chromosome, const uint32_t* start,
                         const uint32_t* end, const uint8_t* strand, const double* posteriormax, const uint8_t* status,
                         const double* meth_lvl, const uint8_t* context);
/* The stable partition of a RESIDENT handle by context, on the device: for every context c of h's mask out3[c] becomes a
 * new, ordinary resident handle of mask 1 << c (every other entry NULL) that holds exactly the records of code c or 3, in
 * file order with their file lines — what abn_sites_parse_dev of the same text with contexts = 1 << c, its deferred lines
 * inserted, holds.  Its chunks keep their slabs' lines; its inserted records and flagged lines are the parent's of that
 * membership; it has no deferred lines.  Only the record counts per (slab, context) come to the host.  h is not consumed;
 * every child is destroyed with abn_sites_destroy (before its context).
 * ABN_ERR_INVALID_ARG: null pointers, a host-form handle, a handle with deferred lines on which abn_sites_insert(_ctx)
 * was never called. */
int abn_sites_split(const abn_sites* h, abn_sites** out3);
/* double[2]: the HIP-event times of abn_sites_split's count and scatter kernels — of the last split of h, or of the
 * split that made h; 0, 0 otherwise */
int abn_sites_split_ms(const abn_sites* h, double* ms2);
/* ---- sorting a resident methylome by genomic position
 * The CANONICAL ORDER is ascending in chromosome key (0..255, M = 256, C = 257), then start, then end, then strand
 * (0 Sense, 1 Antisense, 2 Unknown); equal keys keep their file order.  Inside a chromosome it is the order the
 * alignments ask for, and the chromosomes come in the order of their keys in every sample.
 * abn_sites_sort: the stable radix sort of a RESIDENT handle's sites on the device.  *out becomes a new, ordinary resident
 * handle of h's context and mask that holds exactly h's sites — device records and inserted ones — in canonical order:
 * with order[k] the index of its k-th site in abn_sites_fetch(h), every field of abn_sites_fetch(*out) and of
 * abn_sites_context(*out) is h's at order, and the line of site k is k.  It has one chunk of n_lines = n_sites lines, no
 * deferred lines, counts as inserted, and its flagged lines are the ranks of h's flagged records — what
 * abn_sites_parse_dev with skip_lines 0 holds for the text of h's accepted lines in canonical order.  An input without a
 * descent runs no sort pass.  h is not consumed; *out is destroyed with abn_sites_destroy (before its context).
 * ABN_ERR_INVALID_ARG: null pointers, a host-form handle, a handle with deferred lines on which abn_sites_insert(_ctx)
 * was never called, 2^32 records or more. */
int abn_sites_sort(const abn_sites* h, abn_sites** out);
/* The permutation of a handle abn_sites_sort made: *n its sites, order [*n] the index of every site in the parent's
 * abn_sites_fetch; either may be NULL.
 * ABN_ERR_INVALID_ARG: a null handle, a handle abn_sites_sort did not make. */
int abn_sites_sort_order(const abn_sites* sorted, int64_t* n, int64_t* order);
/* What the sort that made `sorted` did: info4 = {sites, descents (a key below its predecessor's), equal neighbours — both
 * of the input —, radix passes run}; ms4 = the HIP-event times of the flatten, the check, the sort passes and the
 * gather.  Either may be NULL.
 * ABN_ERR_INVALID_ARG: a null handle, a handle abn_sites_sort did not make. */
int abn_sites_sort_info(const abn_sites* sorted, int64_t* info4, double* ms4);
/* The sort itself on one sample's raw key arrays of HOST memory, [n] each: order [n] receives the stable permutation into
 * canonical order, info4 as abn_sites_sort_info.
 * ABN_ERR_INVALID_ARG: null pointers with n > 0, a null info4, n < 0 or n >= 2^32, a chromosome outside 0..257 or a
 * strand above 2 (checked on the host, before any launch). */
int abn_sites_sort_keys(abn_ctx* ctx, int64_t n, const int32_t* chromosome, const uint32_t* start, const uint32_t* end,
                        const uint8_t* strand, int64_t* order, int64_t* info4);
/* ... on DEVICE key arrays (int32, uint32, uint32, uint8); dev_order: uint32 [n] on the device; ms2 (may be NULL) = the
 * HIP-event times of the check and of the sort passes.  Returns after the work has completed.
 * ABN_ERR_INVALID_ARG: as abn_sites_sort_keys; the key ranges are checked by the check kernel, and no pass runs then. */
int abn_sites_sort_keys_dev(abn_ctx* ctx, int64_t n, const void* dev_chromosome, const void* dev_start, const void* dev_end,
                            const void* dev_strand, void* dev_order, int64_t* info4, double* ms2);
/* ---- collapsing the repeated sites of a resident methylome
 * The KEY of a site is (chromosome, start, end, strand), compared as the canonical order compares it.  A RUN is a maximal
 * stretch of consecutive records with equal keys.  The collapse keeps at most one record of every run, by a POLICY, and
 * the kept records keep their order; a run of one record is always kept.
 * PRECONDITION: the input has no descent in canonical order — what abn_sites_sort leaves (its stable sort keeps repeated
 * keys adjacent and in file order) and what a file already in canonical order has.
 *   ABN_DEDUP_FIRST, ABN_DEDUP_LAST  keep the first, the last record of the run in input order: behind abn_sites_sort,
 *                                    in file order
 *   ABN_DEDUP_BEST                   keeps the record with the highest posteriormax.  The run is walked in input order
 *                                    from its first record, and a record replaces the best one so far when
 *                                    better(new, best) = new > best || (isnan(best) && !isnan(new)): ties keep the earlier
 *                                    record, -0.0 and +0.0 tie, a run of only NaN keeps its first record.  The walk is
 *                                    serial in the run's length (the number of replicates of a site)
 *   ABN_DEDUP_DROP                   keeps no record of a run longer than one: a site called twice is not trusted */
#define ABN_DEDUP_FIRST 0
#define ABN_DEDUP_LAST 1
#define ABN_DEDUP_BEST 2
#define ABN_DEDUP_DROP 3
/* abn_sites_dedup: the collapse of a RESIDENT handle's sites on the device.  *out becomes a new, ordinary resident handle
 * of h's context and mask that holds the kept sites of h — device records and inserted ones — in h's order: with order[k]
 * (strictly ascending) the index of its k-th site in abn_sites_fetch(h), every field of abn_sites_fetch(*out) and of
 * abn_sites_context(*out) is h's at order, and the line of site k is k.  It has one chunk of n_lines = n_sites lines, no
 * deferred lines, counts as inserted, and its flagged lines are the ranks of h's flagged records that were kept.  Every
 * builder and abn_sites_split take it as it is.  h is not consumed; *out is destroyed with abn_sites_destroy (before its
 * context).
 * ABN_ERR_INVALID_ARG: null pointers, a host-form handle, a handle with deferred lines on which abn_sites_insert(_ctx)
 * was never called, a policy outside 0..3, 2^32 records or more (before any launch); a descent — abn_last_error names
 * the first descending site and says to sort first —, a chromosome outside 0..257 or a strand above 2 (as
 * abn_sites_sort refuses them). */
int abn_sites_dedup(const abn_sites* h, int policy, abn_sites** out);
/* The kept sites of a handle abn_sites_dedup made: *n its sites, order [*n] the index of every site in the parent's
 * abn_sites_fetch, strictly ascending; either may be NULL.
 * ABN_ERR_INVALID_ARG: a null handle, a handle abn_sites_dedup did not make. */
int abn_sites_dedup_order(const abn_sites* child, int64_t* n, int64_t* order);
/* What the collapse that made `child` did: info4 = {sites of the parent, sites kept, repeated keys (runs longer than
 * one), disagreeing neighbours (adjacent records of equal key whose status U/I/M differs)}; ms4 = the HIP-event times of
 * the flatten, the flags (with the walk of ABN_DEDUP_BEST), the scan (tile counts, their scan, the scatter of the kept
 * indices) and the gather.  Either may be NULL.
 * ABN_ERR_INVALID_ARG: a null handle, a handle abn_sites_dedup did not make. */
int abn_sites_dedup_info(const abn_sites* child, int64_t* info4, double* ms4);
/* The collapse itself on one sample's raw arrays of HOST memory, [n] each: order has room for n entries and receives
 * info4[1] of them, the kept records' indices, ascending; info4 as abn_sites_dedup_info.
 * ABN_ERR_INVALID_ARG: null pointers with n > 0, a null info4, n < 0 or n >= 2^32, a policy outside 0..3, a chromosome
 * outside 0..257 or a strand above 2 (checked on the host, before any launch), a descent. */
int abn_sites_dedup_keys(abn_ctx* ctx, int64_t n, const int32_t* chromosome, const uint32_t* start, const uint32_t* end,
                         const uint8_t* strand, const double* posteriormax, const uint8_t* status, int policy,
                         int64_t* order, int64_t* info4);
/* ... on DEVICE arrays (int32, uint32, uint32, uint8, double, uint8); dev_order: uint32, room for n, on the device; ms2
 * (may be NULL) = the HIP-event times of the flags and of the scan.  Returns after the work has completed.
 * ABN_ERR_INVALID_ARG: as abn_sites_dedup_keys; the key ranges and the descents are found by the flags kernel, and nothing
 * is written to dev_order then. */
int abn_sites_dedup_keys_dev(abn_ctx* ctx, int64_t n, const void* dev_chromosome, const void* dev_start, const void* dev_end,
                             const void* dev_strand, const void* dev_posteriormax, const void* dev_status, int policy,
                             void* dev_order, int64_t* info4, double* ms2);
/* abn_windows_create_sites fed from RESIDENT handles (src/windows.rs:303-339 whole, for n_samples methylomes): sample s is
 * samples[s]; its records and inserted lines are merged in file order on the device into the arrays the gene choice and
 * the placement read — chromosome, start, end, strand, code = status | 0x80 when posteriormax < posterior_max_filter
 * (src/pedigree.rs:165-166), level = meth_lvl — and nothing of per-site size crosses to the host.  The handles are not
 * consumed.  *out is an ordinary abn_windows.
 * ABN_ERR_INVALID_ARG: as abn_windows_create_sites, and a null or host-form sample handle, a handle of another context,
 * a handle with deferred lines on which abn_sites_insert was never called. */
int abn_windows_create_parsed(abn_ctx* ctx, const abn_windows_params* params, abn_genes* genes, const abn_gene_rule* rule,
                              double posterior_max_filter, int32_t n_samples, abn_sites* const* samples,
                              abn_windows** out);
/* double[2]: the HIP-event times of the two merge kernels of abn_windows_create_parsed (the records' fields, the inserted
 * lines: the merge of src/windows.rs:303-338), each over all samples; 0, 0 for a handle made any other way */
int abn_windows_merge_ms(const abn_windows* h, double* ms2);

/* ------------------------------------------------------------------ the pedigree build from RESIDENT handles
 * What Pedigree::build reads of every site, made on the device from n_samples resident handles (abn_sites_parse_dev with
 * skip_lines 0, abn_sites_insert) without a host copy of any site: the packed matrix abn_pairwise_divergence_packed_dev
 * scans, and every sample's rc_meth_lvl fold.  Replaces, behind from_methylome_file_line, the `sites.push` loop and the
 * fold of src/pedigree.rs:147-172 and the status / posterior reads of DMatrix::from (:210-261). */
typedef struct abn_codes abn_codes;
/* src/pedigree.rs:147-172 and :245-251 for n_samples methylomes: sample s is samples[s]; its records and inserted lines
 * are merged in file order on the device, packed (a site is field 3 when posteriormax < posterior_max_filter, :249, else
 * its status) and folded (sum and number of the meth_lvl with posteriormax >= posterior_max_filter, :159-172; a NaN
 * posterior is neither filtered nor counted, as there).  The handles are not consumed.  *out is device-resident until
 * abn_codes_destroy (destroy it before its context).  Samples may differ in length.
 * ABN_ERR_INVALID_ARG, and no handle comes back: a null pointer, n_samples <= 0 or > 65535, a null or host-form sample
 * handle, a handle of another context, a handle with deferred lines on which abn_sites_insert was never called. */
int abn_codes_create_parsed(abn_ctx* ctx, double posterior_max_filter, int32_t n_samples, abn_sites* const* samples,
                            abn_codes** out);
int abn_codes_destroy(abn_codes* h);
/* the shape of the matrix the loop of src/pedigree.rs:210-261 would read: samples, the sites of the longest one, bytes
 * per packed row (abn_packed_row_stride of that, at least 64), same_len = 1 when every sample has that many sites (:221
 * compares the lengths per pair); any pointer may be NULL */
int abn_codes_info(const abn_codes* h, int32_t* n_samples, int64_t* n_sites, int64_t* row_stride_bytes, int32_t* same_len);
/* [n_samples] each, any may be NULL: count = the sample's sites (src/pedigree.rs:147-163); level_sum_kept / kept = the
 * fold of :159-172 before its division, from +0.0 in file order with the host's bits, and the number of its terms */
int abn_codes_stats(const abn_codes* h, int64_t* count, double* level_sum_kept, int64_t* kept);
/* the packed matrix [n_samples x row_stride_bytes] (format above; what abn_pack_codes writes from the code bytes of
 * src/pedigree.rs:245-251, every field behind a sample's last site 3): copied to the host, or its device pointer
 * (16-byte aligned, owned by the handle) */
int abn_codes_packed(abn_codes* h, uint8_t* host_out);
int abn_codes_packed_device_ptr(abn_codes* h, void** dev_ptr);
/* DMatrix::from (src/pedigree.rs:210-261): abn_pairwise_divergence_packed_dev on the resident matrix; HOST outputs
 * [pairs] with abn_pairwise_divergence_packed's order and NULL rules.  Samples that differ in length (:221-227 gives such
 * pairs D = 0 and a message; the caller's business): ABN_ERR_INVALID_ARG with a text that says so, the stats stay valid.
 * n_samples < 2: ABN_OK, nothing is written. */
int abn_codes_pairwise(abn_codes* h, uint64_t* diff, uint64_t* both, double* dvalue);
/* ... and abn_pairwise_transitions_packed_dev on it: HOST table uint64 [pairs x 9]; the same refusal of samples that
 * differ in length.  Under a union alignment the placeholder sites (field 3) count in no entry. */
int abn_codes_transitions(abn_codes* h, uint64_t* table);
/* double[4]: the HIP-event times of abn_codes_create_parsed's kernels (the merge of src/pedigree.rs:147-163 — the
 * records' kernel, the inserted lines' — the pack, the fold), each over all samples */
int abn_codes_kernel_ms(const abn_codes* h, double* ms4);

/* ------------------------------------------------------------------ methylomes aligned by position
 * The reference pairs site k of one methylome with site k of another: src/pedigree.rs:240, "It is assumed that the same
 * sites are included in the datasets".  The entries below lift that assumption: samples are compared on the sites they
 * share.  A site's KEY is (chromosome, start, end, strand) as abn_sites_fetch reports them; the posterior and the status
 * are no part of it, so a filtered site is still a site.  A sample is WELL ORDERED when each chromosome's sites form one
 * contiguous run in file order (the runs in any order) and (start, end, strand) is strictly ascending inside a run.  The
 * COMMON SET is the set of keys present in every sample; every sample keeps its common sites in its own file order; the
 * samples are CO-ORDERED when the k-th common site of every sample has the same key.  One sample: every site is common.
 * A sample without a site: no site is.
 *
 * abn_sites_common lifts src/pedigree.rs:240 for n_samples samples given as HOST arrays (site_offset [n_samples + 1] and
 * per site chromosome, start, end, strand as abn_windows_create_sites takes them): keep [site_offset[n_samples]] = 1 for
 * every sample's common sites, 0 elsewhere; *n_common = their number in each sample.  The step alone, on the device.
 * ABN_ERR_INVALID_ARG: null pointers, n_samples <= 0 or > 65535, site_offset as abn_windows_create, and — with a text
 * that names the sample, the lowest offending site of the whole input (its index inside the sample) and the kind — a
 * sample that is not well ordered ("split run", "not ascending"), a chromosome outside 0..257 or a strand above 2, or
 * samples that are not co-ordered ("not co-ordered"). */
int abn_sites_common(abn_ctx* ctx, int32_t n_samples, const int64_t* site_offset, const int32_t* chromosome,
                     const uint32_t* start, const uint32_t* end, const uint8_t* strand, uint8_t* keep /* uint8 [S] out */,
                     int64_t* n_common /* int64 out */);
/* abn_sites_common (the same lift of src/pedigree.rs:240) on DEVICE arrays; site_offset and n_common stay on the host.
 * Returns after completion. */
int abn_sites_common_dev(abn_ctx* ctx, int32_t n_samples, const int64_t* site_offset, const void* dev_chromosome,
                         const void* dev_start, const void* dev_end, const void* dev_strand, void* dev_keep,
                         int64_t* n_common);
/* abn_windows_create_parsed without the assumption of src/pedigree.rs:240: the merge, then the common-site step, then the
 * gene choice and the placement on the aligned arrays, so that every sample has the same sites in every window and no
 * window is ragged.  Arguments and errors as abn_windows_create_parsed, and the refusals of abn_sites_common (no handle
 * comes back).  The resident handles are neither consumed nor modified.  *out is an ordinary abn_windows; its stats
 * describe the aligned sites. */
int abn_windows_create_aligned(abn_ctx* ctx, const abn_windows_params* params, abn_genes* genes, const abn_gene_rule* rule,
                               double posterior_max_filter, int32_t n_samples, abn_sites* const* samples,
                               abn_windows** out);
/* abn_codes_create_parsed without the assumption of src/pedigree.rs:240: the merge (keys included), the common-site step,
 * then the pack and the fold over the aligned sites.  Arguments and errors as abn_codes_create_parsed, and the refusals of
 * abn_sites_common.  *out is an ordinary abn_codes with same_len = 1 (abn_codes_pairwise works on it); abn_codes_stats
 * reports count = n_common and the folds over the ALIGNED sites, so rc_meth_lvl (p0uu) differs from the unaligned
 * handle's by design. */
int abn_codes_create_aligned(abn_ctx* ctx, double posterior_max_filter, int32_t n_samples, abn_sites* const* samples,
                             abn_codes** out);
/* What the alignment that lifts src/pedigree.rs:240 did to a handle; any pointer may be NULL.  before [n_samples]: every
 * sample's sites as they came; *n_common: the sites every sample keeps; ms [4]: the HIP-event times of the common-site
 * kernels (runs and ends; match; scan and rank; gather).  A handle made any other way: before = the sample's own count,
 * *n_common = -1, ms = zeros. */
int abn_windows_common(const abn_windows* h, int64_t* before /* int64[n] */, int64_t* n_common, double* ms /* double[4] */);
int abn_codes_common(const abn_codes* h, int64_t* before /* int64[n] */, int64_t* n_common, double* ms /* double[4] */);

/* ------------------------------------------------------------------ methylomes aligned on the union of their sites
 * The common set above shrinks with every sample that lacks a site; the comparison the model needs is per pair.
 * DMatrix::from (src/pedigree.rs:240-254) skips a site for a pair when either side's posterior is below the filter and
 * divides by that pair's own compared sites, so a site a sample lacks can stand in its row as a FILTERED PLACEHOLDER.  The
 * entries below give every sample all the sites any sample holds.  KEY and WELL ORDERED as above.  THE UNION ORDER: inside
 * a chromosome the distinct keys ascend by (start, end, strand); the chromosomes come in the run order of the REFERENCE
 * SAMPLE (the one with the most runs, the lowest index among equals), those it lacks behind them in the order they are
 * first met going through the samples 0 .. n-1, each in its run order.  Every sample's run order must be a subsequence of
 * that order.  n_union is the number of distinct keys; after the step every sample has n_union sites: site u is the
 * sample's own site with the key of union rank u, or the placeholder — that key, code 0x80 (status U, filtered; as a
 * merged byte of the codes form: not counted for rc_meth_lvl), level +0.0.  The result is what the unaligned entries give
 * on input into which, for every key a sample lacks, a row with that key, status U, posteriormax 0 and level 0 was
 * inserted at its place in the union order (with a posterior filter above 0).  A sample without a site becomes a row of
 * placeholders.  All sites together must be fewer than 2^32, hence n_union too.
 *
 * abn_sites_union is the step alone for the per-pair comparison of src/pedigree.rs:240-254, on HOST arrays (arguments as
 * abn_sites_common): dest [site_offset[n_samples]] = every site's union rank, *n_union = the distinct keys.
 * ABN_ERR_INVALID_ARG: as abn_sites_common for the arguments, "split run", "not ascending" and a key outside its range
 * (the same texts), and "run order": a run whose chromosome stands in the union order before the chromosome of the
 * sample's run in front of it, named by its sample and its first site; the lowest offending site of the whole input
 * decides among several violations of the well-ordering, and among several of the run order. */
int abn_sites_union(abn_ctx* ctx, int32_t n_samples, const int64_t* site_offset, const int32_t* chromosome,
                    const uint32_t* start, const uint32_t* end, const uint8_t* strand, uint32_t* dest /* uint32 [S] out */,
                    int64_t* n_union /* int64 out */);
/* abn_sites_union (src/pedigree.rs:240-254 per pair) on DEVICE arrays; site_offset and n_union stay on the host.  Returns
 * after completion. */
int abn_sites_union_dev(abn_ctx* ctx, int32_t n_samples, const int64_t* site_offset, const void* dev_chromosome,
                        const void* dev_start, const void* dev_end, const void* dev_strand, void* dev_dest,
                        int64_t* n_union);
/* abn_windows_create_parsed for samples that hold different sites, compared pair by pair as src/pedigree.rs:240-254 does:
 * the merge, then the union step, then the gene choice and the placement on n_samples x n_union sites.  Every sample has
 * the same sites in every window, so no window is ragged; count counts union sites, kept and level_sum_kept are those of
 * the sample's own sites, level_sum counts a placeholder as a site of level 0.  Arguments and errors as
 * abn_windows_create_parsed, and the refusals of abn_sites_union (no handle comes back).  The resident handles are neither
 * consumed nor modified. */
int abn_windows_create_union(abn_ctx* ctx, const abn_windows_params* params, abn_genes* genes, const abn_gene_rule* rule,
                             double posterior_max_filter, int32_t n_samples, abn_sites* const* samples,
                             abn_windows** out);
/* abn_codes_create_parsed for samples that hold different sites (src/pedigree.rs:240-254 per pair): the merge (keys
 * included), the union step, then the pack and the fold over n_union sites per sample.  *out is an ordinary abn_codes with
 * same_len = 1; abn_codes_stats reports count = n_union, and kept and level_sum_kept with the bits of the unaligned
 * handle's: a placeholder is not counted.  D of a pair is over the sites both samples hold and both pass the filter.
 * Arguments and errors as abn_codes_create_parsed, and the refusals of abn_sites_union. */
int abn_codes_create_union(abn_ctx* ctx, double posterior_max_filter, int32_t n_samples, abn_sites* const* samples,
                           abn_codes** out);
/* What the union alignment (src/pedigree.rs:240-254 per pair) did to a handle; any pointer may be NULL.  before
 * [n_samples]: every sample's sites as they came; *n_union: the sites every sample has now; ms [8]: the HIP-event times
 * of the passes (runs and ends; owner; scan; base; rank; dest; invert; gather).  A handle made any other way: *n_union =
 * -1, ms = zeros; abn_windows_common / abn_codes_common report n_common = -1 on a union handle. */
int abn_windows_union(const abn_windows* h, int64_t* before /* int64[n] */, int64_t* n_union, double* ms /* double[8] */);
int abn_codes_union(const abn_codes* h, int64_t* before /* int64[n] */, int64_t* n_union, double* ms /* double[8] */);

/* Genomic tiles: Pedigree::build (src/pedigree.rs:147-172, :210-261) once per tile of the genome — a fixed bin, or a row of
 * a region list such as the chromatin-state rows src/cli/metaprofile.rs:50-72 reads — over resident parse results.  The
 * handle does what abn_codes_create_parsed / _aligned / _union do (align 0 none, 1 position, 2 union) and keeps, beside the
 * packed matrix, the columns' keys (chromosome, start: one copy, all samples share them after the alignment), every
 * sample's merged bytes and levels, and the chromosome runs of the columns.  align 0 is the reference's assumption
 * (src/pedigree.rs:240): the keys are sample 0's, every sample must have sample 0's number of sites
 * (ABN_ERR_INVALID_ARG, the text names --align), and sample 0 must be well ordered (the refusals of abn_sites_common).
 * Arguments and errors otherwise as abn_codes_create_parsed.
 *
 * A tile is (chromosome 0..257, start, end) with start, end in [0, 2^32], half-open on a site's start; the strand is no
 * part of it.  Its columns [begin, end) come from two lower bounds inside the chromosome's run; begin = end for a
 * chromosome without a run, for end <= start, and behind the last site.  abn_tiles_set_intervals takes a list,
 * abn_tiles_set_fixed makes one from the runs: for every run in run order the tiles k = 0 .. ceil((last_start + 1) / step)
 * - 1, [k step, k step + size) (step 0: size; the end capped at 2^32; tiles overlap when step < size).  Either runs the
 * search and the per-(sample, tile) folds on the device, may be called again (the new list replaces the old) and refuses
 * with ABN_ERR_INVALID_ARG: null pointers, n_tiles < 0, a chromosome outside 0..257, a bound outside [0, 2^32], size <= 0,
 * step < 0, more tiles than INT32_MAX.  The getters of tiles refuse before any set_*.
 *
 * abn_tiles_stats: count [T] = the tile's columns; level_sum_kept, kept [n x T] = the fold of src/pedigree.rs:159-172 over
 * the tile's sites of the sample alone, bit for bit (a union placeholder is filtered and not counted).
 * abn_tiles_pairwise: abn_pairwise_divergence_windows_packed_dev over the tiles' column ranges, host outputs [T x pairs]
 * (any may be NULL; fewer than two samples: nothing is written).  abn_tiles_kernel_ms: double[2], the HIP-event times of
 * the last set_*'s search and fold. */
typedef struct abn_tiles abn_tiles;
int abn_tiles_create(abn_ctx* ctx, double posterior_max_filter, int32_t align /* 0 none, 1 position, 2 union */,
                     int32_t n_samples, abn_sites* const* samples, abn_tiles** out);
int abn_tiles_destroy(abn_tiles* h);
int abn_tiles_info(const abn_tiles* h, int32_t* n_samples, int64_t* n_columns, int64_t* row_stride_bytes, int32_t* n_runs,
                   int64_t* n_tiles /* -1 before any set_* */);
/* the runs in run order, [n_runs] each: chromosome, first column, columns, the start of the last column */
int abn_tiles_runs(const abn_tiles* h, int32_t* chromosome, int64_t* first, int64_t* count, uint32_t* last_start);
int abn_tiles_set_intervals(abn_tiles* h, int64_t n_tiles, const int32_t* chromosome, const int64_t* start,
                            const int64_t* end);
int abn_tiles_set_fixed(abn_tiles* h, int64_t size, int64_t step /* 0: size */);
int abn_tiles_intervals(const abn_tiles* h, int32_t* chromosome, int64_t* start, int64_t* end); /* [n_tiles] */
int abn_tiles_layout(const abn_tiles* h, int64_t* begin, int64_t* end);                         /* [n_tiles] */
int abn_tiles_stats(const abn_tiles* h, int64_t* count /* [T] */, double* level_sum_kept /* [n x T] */,
                    int64_t* kept /* [n x T] */);
int abn_tiles_pairwise(abn_tiles* h, uint64_t* diff, uint64_t* both, double* dvalue); /* host, [T x pairs] */
/* abn_pairwise_transitions_windows_packed_dev over the matrix and ranges abn_tiles_pairwise scans (with pools set: the
 * pooled matrix, one table per pool): HOST table uint64 [T x pairs x 9] */
int abn_tiles_transitions(abn_tiles* h, uint64_t* table);
int abn_tiles_kernel_ms(const abn_tiles* h, double* ms2 /* search, fold */);

/* Region pools: one pedigree per annotation CLASS — every gene, every TE, each chromatin state of a list such as the rows
 * src/cli/metaprofile.rs:50-72 reads — where abn_tiles_set_intervals makes one per row; stands in for cutting every
 * methylome into per-class files on the host and Pedigree::build (src/pedigree.rs:147-172, :210-261) on each.
 * abn_tiles_set_pools: interval k = (chromosome, start, end)[k], as a tile's, belongs to pool[k] in [0, n_pools).  A pool's
 * columns are the handle's columns whose (chromosome, start) lies in at least one of its intervals, each once, in ascending
 * column order (under align 0: the order of the lines in every sample's file); an interval may belong to several pools by
 * being listed for each.  Per pool the intervals are merged — chromosomes in the run order of the columns, one without a
 * run and intervals with end <= start dropped, overlapping or touching intervals joined — into SEGMENTS, whose columns are
 * gathered on the device into a pooled matrix and pooled merged bytes and levels.  Afterwards the handle's tiles are the
 * pools: abn_tiles_info reports n_tiles = n_pools, abn_tiles_layout every pool's range in POOLED column space,
 * abn_tiles_stats and abn_tiles_pairwise the pools' folds and scans, abn_tiles_kernel_ms the search (of the segments) and
 * the fold, abn_tiles_pool_kernel_ms double[4]: offsets, map, gather, pack.  A pool without a column is an empty tile, no
 * error.  abn_tiles_intervals refuses on such a handle (ABN_ERR_INVALID_ARG; the text names abn_tiles_pool_segments).
 * A later abn_tiles_set_intervals / _set_fixed puts the handle back on its own matrix, and the other way round.
 * ABN_ERR_INVALID_ARG, the handle as it was: null pointers, n_intervals < 0, n_pools <= 0 or above INT32_MAX, a pool id
 * outside [0, n_pools) (the text names the interval), an interval abn_tiles_set_intervals refuses, a pooled matrix beyond
 * the limits of a handle's own ("too large for one handle").
 * abn_tiles_pool_segments: *n_segments and, [n_segments] each in segment order (pool by pool, ascending columns inside
 * one), the segment's pool, its merged interval and its columns [col_begin, col_end) of the handle's own matrix.
 * abn_tiles_pool_columns: src [the last pool's layout end] = every pooled column's source column.  Any output may be NULL. */
int abn_tiles_set_pools(abn_tiles* h, int64_t n_intervals, const int32_t* chromosome, const int64_t* start,
                        const int64_t* end, const int32_t* pool, int64_t n_pools);
int abn_tiles_pool_segments(const abn_tiles* h, int64_t* n_segments, int32_t* pool, int32_t* chromosome, int64_t* start,
                            int64_t* end, int64_t* col_begin, int64_t* col_end);
int abn_tiles_pool_columns(const abn_tiles* h, int64_t* src);
int abn_tiles_pool_kernel_ms(const abn_tiles* h, double* ms4 /* offsets, map, gather, pack */);

/* Block bootstrap: the uncertainty of a rate estimated for a pool of regions or a tiled genome, where the reference has only
 * the residual bootstrap of one pedigree's rows (src/boot_model.rs:43-57; the observed site counts stay fixed there).  T
 * blocks in G groups, group g the contiguous ascending block range [group_begin[g], group_end[g]); per group R + 1 rows of
 * counts, rows 0 .. R - 1 drawn with replacement (draw j of row r: block group_begin + index_from(word j % 4 of
 * philox4x32_10(j / 4, r, group_id[g], 4, seed_lo, seed_hi), T_g): a row depends on neither R nor G), row R the identity row
 * of ones.  Every row's sums stand in for DMatrix::from and the rc_meth_lvl fold over the drawn blocks' sites
 * (src/pedigree.rs:236-257, :159-172): both* = sum_t c both[t], diff* likewise (exact), dvalue* = diff* / (2 both*) (0 / 0 is
 * NaN), level* = sum_t (double)c level_sum_kept[s][t] serially in ascending t (product, then add), kept* = sum_t c kept[s][t].
 * Tables: both, diff uint64 [T x P]; level_sum_kept double, kept int64 [n x T].  Counts: uint8 [G x rows x T], group-major,
 * read inside a group's range alone.  Outputs: both_out, diff_out, dvalue_out [G x rows x P], level_out, kept_out
 * [G x rows x n]; any may be NULL.  ABN_ERR_INVALID_ARG with a text, before any launch: a table value >= 2^35, a group of
 * more than 2^21 blocks, R > 2^20 - 2, G > 4096, null pointers, negative sizes, unordered or overlapping group ranges, a
 * count above 127 (abn_block_counts: raised by the kernel, probability below 1e-200; device arguments: found by the
 * kernels, the outputs are then no result).  An empty group is no error: sums 0, dvalue NaN.
 * abn_block_counts: the counts of R replicates and the identity row, made on the device, to the HOST buffer counts
 * [G x (R + 1) x n_blocks], zero outside a group's range.  abn_block_counts_host: its serial form, no device; `text`
 * (text_bytes, may be NULL) takes a refusal's text.
 * abn_block_resample: explicit counts (a jackknife's as well) and HOST buffers.  abn_block_resample_dev: the same on DEVICE
 * pointers (group_begin and group_end stay host arrays), ms5 (may be NULL): the HIP-event times of counts (0 here), digits,
 * product, finish, levels.  abn_block_resample_host: the serial form, no device, refusals as abn_block_counts_host. */
int abn_block_counts(abn_ctx* ctx, uint64_t seed, int32_t n_groups, const uint32_t* group_id, const int64_t* group_begin,
                     const int64_t* group_end, int64_t n_replicates, int64_t n_blocks, uint8_t* counts);
int abn_block_counts_host(uint64_t seed, int32_t n_groups, const uint32_t* group_id, const int64_t* group_begin,
                          const int64_t* group_end, int64_t n_replicates, int64_t n_blocks, uint8_t* counts, char* text,
                          int32_t text_bytes);
int abn_block_resample(abn_ctx* ctx, int32_t n_groups, const int64_t* group_begin, const int64_t* group_end,
                       int64_t rows_per_group, const uint8_t* counts, int64_t n_blocks, int64_t n_pairs, int32_t n_samples,
                       const uint64_t* both, const uint64_t* diff, const double* level_sum_kept, const int64_t* kept,
                       uint64_t* both_out, uint64_t* diff_out, double* dvalue_out, double* level_out, int64_t* kept_out);
int abn_block_resample_dev(abn_ctx* ctx, int32_t n_groups, const int64_t* group_begin, const int64_t* group_end,
                           int64_t rows_per_group, const void* dev_counts, int64_t n_blocks, int64_t n_pairs,
                           int32_t n_samples, const void* dev_both, const void* dev_diff, const void* dev_level_sum_kept,
                           const void* dev_kept, void* dev_both_out, void* dev_diff_out, void* dev_dvalue_out,
                           void* dev_level_out, void* dev_kept_out, double* ms5);
int abn_block_resample_host(int32_t n_groups, const int64_t* group_begin, const int64_t* group_end, int64_t rows_per_group,
                            const uint8_t* counts, int64_t n_blocks, int64_t n_pairs, int32_t n_samples, const uint64_t* both,
                            const uint64_t* diff, const double* level_sum_kept, const int64_t* kept, uint64_t* both_out,
                            uint64_t* diff_out, double* dvalue_out, double* level_out, int64_t* kept_out, char* text,
                            int32_t text_bytes);
/* The block bootstrap of a tiles handle, HOST outputs [G x (R + 1) x pairs] and [G x (R + 1) x n] (any may be NULL).  With
 * pools set the blocks are the pools' merged segments in abn_tiles_pool_segments order and the groups the pools (group_id =
 * pool); after abn_tiles_set_fixed with step 0 or step >= size the blocks are the tiles, one group of id 0.  The blocks'
 * tables come from the windows scan and the per-(sample, block) fold over the handle's own matrix and never leave the
 * device.  Refused (ABN_ERR_INVALID_ARG) after abn_tiles_set_intervals and after a fixed tiling with 0 < step < size: the
 * blocks may overlap.  abn_tiles_block_ms: double[5], the HIP-event times of the last call's counts, digits, product,
 * finish and levels. */
int abn_tiles_block_bootstrap(abn_tiles* h, uint64_t seed, int64_t n_replicates, uint64_t* both_out, uint64_t* diff_out,
                              double* dvalue_out, double* level_out, int64_t* kept_out);
/* the groups of that call in block space: *n_groups, *n_blocks and [n_groups] the groups' block ranges (any may be NULL) */
int abn_tiles_block_groups(const abn_tiles* h, int64_t* n_groups, int64_t* n_blocks, int64_t* group_begin,
                           int64_t* group_end);
int abn_tiles_block_ms(const abn_tiles* h, double* ms5);

/* Region-level states of a tiles handle: abn_packed_region_states_dev (the law above, the library's long_sites) over the
 * handle's own matrix with the handle's tiles — as abn_tiles_set_intervals or abn_tiles_set_fixed left them — as the
 * windows.  group [n_tiles] (NULL: all 0) puts tile t into group[t] in [0, n_groups), -1 leaves the tile out; the output
 * columns are the tiles in ascending (group, tile index), so every group is one contiguous column range — one region-level
 * pedigree per group.  The new handle owns its matrix and is independent of later changes to h.  ABN_ERR_INVALID_ARG:
 * before any set_*; with pools set (a pool is a class of sites, not a region); n_groups < 1; a group outside
 * [-1, n_groups) (the text names the tile); a rule outside the law's bounds.  An empty group is no error: zeros and NaN, as
 * an empty window gets; nor is a matrix without any column (every tile left out).
 * abn_regions_info: any output may be NULL; row_stride_bytes = abn_packed_row_stride(n_columns), at least 64.
 * abn_regions_layout: group_begin, group_end [n_groups], in columns.  abn_regions_order: src [n_columns], the tile of each
 * column.  abn_regions_packed: the matrix [n_samples x row_stride_bytes] to the host; _device_ptr: where it lives.
 * abn_regions_census: abn_packed_census_windows_dev over the groups' ranges, HOST counts uint64 [n_groups x n_samples x 3].
 * abn_regions_pairwise: abn_pairwise_divergence_windows_packed_dev over them, host outputs [n_groups x pairs] (any may be
 * NULL); abn_regions_transitions: HOST table uint64 [n_groups x pairs x 9].  abn_regions_kernel_ms: double[2], the HIP-event
 * times of the long tiles' census and of the kernel. */
typedef struct abn_regions abn_regions;
int abn_tiles_region_states(abn_tiles* h, int64_t lo_num, int64_t hi_num, int64_t den, int64_t min_kept,
                            const int32_t* group /* [n_tiles], NULL: all 0; -1: the tile is left out */, int32_t n_groups,
                            abn_regions** out);
int abn_regions_destroy(abn_regions* h);
int abn_regions_info(const abn_regions* h, int32_t* n_samples, int64_t* n_columns, int64_t* row_stride_bytes,
                     int32_t* n_groups);
int abn_regions_layout(const abn_regions* h, int64_t* group_begin, int64_t* group_end);
int abn_regions_order(const abn_regions* h, int32_t* src);
int abn_regions_packed(abn_regions* h, uint8_t* host_out);
int abn_regions_packed_device_ptr(abn_regions* h, void** dev_ptr);
int abn_regions_census(abn_regions* h, uint64_t* counts);
int abn_regions_pairwise(abn_regions* h, uint64_t* diff, uint64_t* both, double* dvalue);
int abn_regions_transitions(abn_regions* h, uint64_t* table);
int abn_regions_kernel_ms(const abn_regions* h, double* ms2);

/* ------------------------------------------------------------------ (4) batched, device-resident plan
 * One pedigree topology (t0,t1,t2 of N rows), W windows that differ in D / p0uu (the metaprofile loop,
 * src/cli/metaprofile.rs:50-72, where every window shares nodelist/edgelist), S starts and B bootstraps
 * per window.  boot_offset / window_offset place this plan's shard in the global (window, bootstrap)
 * index space so that results do not depend on how the job is sharded over GPUs. */
int abn_plan_create(abn_ctx* ctx, const abn_options* opts, const double* generations /* N x 3 */,
                    int32_t n_rows, int32_t n_windows, int32_t n_starts, int32_t n_boot,
                    uint32_t window_offset, uint32_t boot_offset, abn_plan** plan);
int abn_plan_destroy(abn_plan* plan);
/* Optional, before abn_plan_set_windows: ids[W] = each window's index in the Philox counters (start simplices,
 * jitter, bootstrap indices).  Default: window_offset + w.  The metaprofile driver passes every window's own
 * position in the (region, window) enumeration (src/cli/metaprofile.rs:50-53), so that skipped windows and
 * several topology groups never make two windows share a random stream.  NULL restores the default. */
int abn_plan_set_window_ids(abn_plan* plan, const uint32_t* ids);
/* D[W x N], p0uu[W]; eqp = p0uu and eqp_weight = 1 as src/alphabeta.rs:33-54 unless eqp/eqp_weight
 * are non-NULL ([W] each).  Also draws the start simplices and generates the bootstrap index buffer
 * idx[W x B x N] (u32) in HBM on the device. */
int abn_plan_set_windows(abn_plan* plan, const double* d_obs, const double* p0uu, const double* eqp,
                         const double* eqp_weight);
/* enqueue phase A (starts) -> select -> phase B (bootstraps) on the context's stream; asynchronous */
int abn_plan_run(abn_plan* plan);
int abn_plan_run_phase(abn_plan* plan, int32_t phase /* 0 = A+select, 1 = B */);
int abn_plan_sync(abn_plan* plan);
/* Diagnostics: out2 = chains the last persistent (queue + time-sliced) launch of phase A / phase B handed to its tail — the
 * last chains of such a launch finish on abn_fit_spec_kernel (four wavefronts per chain) instead of one by one on an
 * emptying GPU; 0 when the phase did not run persistent.  Same bits either way.  Synchronises like abn_plan_sync. */
int abn_plan_tail_handed(abn_plan* plan, int64_t* out2);
/* Early bootstraps.  Phase B needs a window's BEST start, not its slowest: on a plan of one window with at least five
 * starts (auto options, no window groups) whose starts run on abn_fit_spec_kernel and whose bootstraps run on the
 * persistent kernel, abn_plan_run launches phase B once a quorum of the starts has finished; the others finish beside it,
 * and phase B is stopped and redone when one of them turns out best (a "miss").  Results are the same bytes either way.
 * mode: 0 = off, 1 = auto (the default).  abn_plan_run_phase never does this. */
int abn_plan_set_early_bootstraps(abn_plan* plan, int32_t mode);
/* out4 = the plan is eligible (0 / 1), its quorum, and of the last abn_plan_run (0 when it did not launch phase B early):
 * starts that were still running at the quorum, miss (0 / 1).  Synchronises like abn_plan_sync. */
int abn_plan_early_bootstraps(abn_plan* plan, int32_t* out4);
/* Streamed pedigrees: sweep a chain's rows once per Nelder-Mead iteration instead of once per cost evaluation — the
 * reflection, the expansion and the contraction of an iteration are evaluated in one pass, each with the additions of the
 * per-evaluation kernel in the same order.  Results are the same bytes either way.  mode: 0 = off (the default), 1 = both
 * phases of later abn_plan_run / abn_plan_run_phase calls take the sweep kernel where the launch streams with one wavefront
 * per chain in tree order and one pass; every other launch runs what it runs at mode 0. */
int abn_plan_set_stream_sweep(abn_plan* plan, int32_t mode);
/* out4 = the mode, whether phase A of the last run used the sweep kernel (0 / 1), the same for phase B, and the passes
 * over the rows its sweep launches counted.  Synchronises like abn_plan_sync. */
int abn_plan_stream_sweep(abn_plan* plan, int64_t* out4);
/* HIP-event time of the most recent launch of each kernel, in milliseconds (fit A, select, fit B) */
int abn_plan_kernel_ms(abn_plan* plan, double* ms3);
/* device pointer of raw[W x B x 7] (for an RCCL gather by the caller) and optional rebinding to a
 * caller-owned device buffer of the same size */
int abn_plan_raw_device_ptr(abn_plan* plan, void** dev_ptr);
int abn_plan_bind_raw(abn_plan* plan, void* dev_ptr);
/* copy results to the host; any pointer may be NULL.  models[W x 4], pred[W x N], resid[W x N],
 * raw[W x B x 7], info_a[W x S], info_b[W x B], best_start[W] (int32, -1 = no start of that window ended finite).
 * Returns ABN_ERR_NO_FINITE_FIT — AFTER filling every buffer — when any window has best_start = -1 (the reference
 * panics, src/ab_neutral.rs:28,100; metaprofile prints and skips the window, src/cli/metaprofile.rs:64-65): that
 * window's model, pred, resid and bootstrap rows are NaN, the other windows are valid. */
int abn_plan_download(abn_plan* plan, double* models, double* pred, double* resid, double* raw,
                      abn_fit_info* info_a, abn_fit_info* info_b, int32_t* best_start);
/* src/analysis.rs:50-98 of every window of the plan, on the device (abn_analyze_batch_dev on the table the plan currently
 * writes — its own or the one given to abn_plan_bind_raw — so only W x 32 doubles come back instead of raw[W x B x 7]):
 * out[W x 32], first_bad[W] (may be NULL) are HOST arrays.  ABN_ERR_STATE when phase B has not run;
 * ABN_ERR_NO_FINITE_FIT after filling every buffer when a window's table holds a NaN (a window without a finite start
 * among them).  Synchronises like abn_plan_sync. */
int abn_plan_analyze(abn_plan* plan, double* out, int32_t* first_bad);
/* number of windows whose selection found no finite start in the last phase-A run (cheap: W int32 come back) */
int abn_plan_failed_windows(abn_plan* plan, int32_t* n_failed);
/* sums over all fits of the last run (for evals/s): out[0] = fits, out[1] = evals (cost() calls of the reference
 * algorithm = sum of abn_fit_info.evals), out[2] = iters, out[3] / out[4] = evaluations of out[1] in the start / bootstrap
 * fits that were NOT executed because the fit had reached a fixed point (options.no_fixed_point_skip) */
int abn_plan_counters(abn_plan* plan, int64_t* out5);
/* number of bytes of device memory the plan holds (index buffer included) */
int abn_plan_device_bytes(abn_plan* plan, int64_t* bytes);
/* which fit kernel the last run of each phase used (the choice depends on the size of the launch, never the bits):
 * out[0] = kernel of phase A (ABN_KERNEL_*), out[1] = its lanes per chain, out[2] / out[3] the same for phase B */
#define ABN_KERNEL_NONE 0         /* the phase has not run                                                   */
#define ABN_KERNEL_SPECULATIVE 1  /* four wavefronts per chain (few chains: latency-bound)                   */
#define ABN_KERNEL_RESIDENT 2     /* one launch, pedigree in LDS; lanes = 64: a wavefront per chain          */
#define ABN_KERNEL_PERSISTENT 3   /* resident, persistent wavefronts with a chain queue and time slicing     */
#define ABN_KERNEL_STREAM 4       /* rows re-read from HBM every evaluation                                  */
#define ABN_KERNEL_TWO_PASS 5     /* resident, long chains parked and resumed in a second launch             */
#define ABN_KERNEL_STREAM_SWEEP 6 /* streamed, rows read once per iteration (abn_plan_set_stream_sweep)      */
int abn_plan_last_kernels(abn_plan* plan, int32_t* out4);

/* ------------------------------------------------------------------ (5) one process, several GPUs of a node
 * The metaprofile loop (src/cli/metaprofile.rs:50-72) over all MI355X of a node from ONE host thread: a plan per
 * device on a stream of its own (the devices run concurrently), windows dealt in contiguous blocks — or, with fewer
 * windows than devices, every device repeats the cheap phase A (same inputs, same bits) and takes a contiguous slice
 * of the bootstraps.  Every fit is independent and every random draw is a function of the GLOBAL (window,
 * bootstrap) index, and the reduction tree is the pedigree's (abn_options.lanes_per_chain): the tables are
 * byte-identical for every number of devices.  abn_multi_run ends with the one exchange step of the path: the
 * gather of the bootstrap tables (56 B per fit) into every device's copy of raw[W x B x 7] over xGMI with RCCL
 * (in-place ncclAllGather for equal window blocks, else ncclBroadcast per block), enqueued behind the kernels on
 * each device's stream.  RCCL is bound at run time (librccl.so.1) and only when n_devices > 1.
 * devices[n_devices]: distinct HIP ordinals.  On failure *out may be non-NULL (abn_multi_last_error explains it)
 * and must still be destroyed. */
typedef struct abn_multi abn_multi;
int abn_multi_create(const int32_t* devices, int32_t n_devices, const abn_options* opts,
                     const double* generations /* N x 3 */, int32_t n_rows, int32_t n_windows, int32_t n_starts,
                     int32_t n_boot, abn_multi** out);
int abn_multi_destroy(abn_multi* m);
const char* abn_multi_last_error(const abn_multi* m);
/* ids[W] for ALL windows, before abn_multi_set_windows (as abn_plan_set_window_ids); NULL restores the default */
int abn_multi_set_window_ids(abn_multi* m, const uint32_t* ids);
/* abn_plan_set_stream_sweep on every device's plan */
int abn_multi_set_stream_sweep(abn_multi* m, int32_t mode);
/* D[W x N], p0uu[W], optional eqp[W], eqp_weight[W] for ALL windows (as abn_plan_set_windows) */
int abn_multi_set_windows(abn_multi* m, const double* d_obs, const double* p0uu, const double* eqp,
                          const double* eqp_weight);
/* A -> select -> B on every device, then the gather; asynchronous */
int abn_multi_run(abn_multi* m);
int abn_multi_sync(abn_multi* m);
/* out4 = window_offset, n_windows, boot_offset, n_boot of the shard of devices[device_index] */
int abn_multi_shard(abn_multi* m, int32_t device_index, int32_t* out4);
/* the same partition as host arithmetic, no device or handle needed: which windows / bootstraps device
 * `device_index` of `n_devices` takes (contiguous balanced blocks of windows; with fewer windows than devices every
 * device takes all windows and a block of the bootstraps) — the rule of the one-process-per-GPU path too */
int abn_multi_plan_shard(int32_t n_windows, int32_t n_boot, int32_t n_devices, int32_t device_index, int32_t* out4);
/* HIP-event milliseconds of devices[device_index]'s last run: ms3 = (phase A, selection, phase B), as abn_plan_kernel_ms */
int abn_multi_kernel_ms(abn_multi* m, int32_t device_index, double* ms3);
/* the gathered table raw[W x B x 7] in the memory of devices[device_index] (valid after abn_multi_sync) */
int abn_multi_raw_device_ptr(abn_multi* m, int32_t device_index, void** dev_ptr);
/* as abn_plan_download for all W windows (raw comes from the first device's gathered table); returns
 * ABN_ERR_NO_FINITE_FIT after filling every buffer when a window has no finite start */
int abn_multi_download(abn_multi* m, double* models, double* pred, double* resid, double* raw,
                       abn_fit_info* info_a, abn_fit_info* info_b, int32_t* best_start);
/* src/analysis.rs:50-98 of all W windows on the first device's gathered table (as abn_plan_analyze; valid after
 * abn_multi_run, synchronises like abn_multi_sync): out[W x 32], first_bad[W] (may be NULL), HOST arrays */
int abn_multi_analyze(abn_multi* m, double* out, int32_t* first_bad);
/* abn_plan_counters summed over the devices (bootstrap-sharded mode: the replicated phase-A fits count per device) */
int abn_multi_counters(abn_multi* m, int64_t* out5);
/* *ok = 1 when librccl.so.1 can be loaded and exports every symbol the gather uses */
int abn_multi_rccl_available(int* ok);

/* ------------------------------------------------------------------ methylomes simulated down a pedigree
 * The ABneutral model run forwards (src/divergence.rs:33-114): a site of a diploid selfing line is UU, UM or MM (codes 0,
 * 1, 2: the U / I / M of DMatrix::from, src/pedigree.rs:253-257); one generation applies genmatrix(alpha, beta) (:96-114);
 * the founder is drawn from [p_uu, w p_mm, (1 - w) p_mm] (:44).  The model's dt1t2 of a pair (:68-89) is E|s_i - s_j| / 2 of
 * two lineages that split at t0, the quantity DMatrix::from measures.  The reference has no generator: its end-to-end tests
 * are commented out (src/alphabeta.rs:81-140, src/ab_neutral.rs:144-161).
 * A tree of n_nodes nodes: parent[0] = -1, 0 <= parent[v] < v; thr uint64 [n_nodes][3][2], thr[v][s][0] <= thr[v][s][1];
 * emit uint8 [n_nodes].  The draw of site k at node v: u = (uint64)H[k & 3] << 32 | Lw[k & 3], H = philox4x32_10(c0 =
 * (uint32)(k >> 2), c1 = 0, c2 = v, c3 = 5, seed_lo, seed_hi), Lw the same call with c1 = 1.  The founder's state is
 * (u >= thr[0][0][0]) + (u >= thr[0][0][1]); any other node's, with s its parent's state at the site,
 * (u >= thr[v][s][0]) + (u >= thr[v][s][1]).  The r-th emitted node, in node order, is row r of a packed matrix (format
 * above): the field of site k its state, every field from n_sites to the end of abn_packed_row_stride(n_sites) bytes 3;
 * bytes of a longer row_stride_bytes are not written.  A row depends on the seed, the node's index, its ancestors and their
 * thresholds alone.
 * ABN_ERR_INVALID_ARG with a text, before any launch: null pointers, n_nodes < 1 or > 65535 (what the pairwise scan takes
 * as samples), a parent outside the rule, thr[..][0] > thr[..][1], no emitted node, n_sites < 0 or > 2^34, a
 * row_stride_bytes that is not a multiple of 64 or is below abn_packed_row_stride(n_sites).
 *
 * abn_sim_thresholds (host arithmetic, no device; src/divergence.rs:16-31, :44, :55, :96-114): thr from rates.  For v > 0
 * the rows of G^(generation[v] - generation[parent[v]]), G = genmatrix(alpha, beta), the power the reference's
 * left-accumulated chain (power 0: the identity); the founder's row [p_uu0, w (1 - p_uu0), (1 - w)(1 - p_uu0)] .
 * G^generation[0].  Of a row p: c0 = p[0], c1 = p[0] + p[1]; threshold(c) = 0 for c <= 0, 2^64 - 1 for c >= 1, else
 * (uint64)ldexp(c, 64).  A cumulative probability is resolved to 2^-53: a one-generation UU -> MM step at alpha = 4e-9
 * (1.6e-17) cannot be represented.  `text` (text_bytes, may be NULL) takes a refusal's text.  ABN_ERR_INVALID_ARG: null
 * pointers, n_nodes < 1 or > 65535, a parent outside the rule, a generation outside 0..127 (the reference's i8,
 * src/divergence.rs:52), a child older than its parent, alpha, beta, p_uu0 or weight outside [0, 1] or not finite. */
int abn_sim_thresholds(double alpha, double beta, double p_uu0, double weight, int32_t n_nodes, const int32_t* parent,
                       const int32_t* generation, uint64_t* thr, char* text, int32_t text_bytes);
/* The launch abn_sim_codes* makes for n_sites sites on this context (src/divergence.rs:33-114 has no counterpart): grid2 =
 * {workgroups, lanes per workgroup}; a lane owns one dword (16 sites) of a row per trip of its grid stride. */
int abn_sim_grid(abn_ctx* ctx, int64_t n_sites, int32_t* grid2);
/* The simulation (src/divergence.rs:33-114 forwards) to the HOST matrix packed [emitted nodes x row_stride_bytes]. */
int abn_sim_codes(abn_ctx* ctx, uint64_t seed, int32_t n_nodes, const int32_t* parent, const uint64_t* thr,
                  const uint8_t* emit, int64_t n_sites, uint8_t* packed, int64_t row_stride_bytes);
/* ... to the DEVICE matrix dev_packed (16-byte aligned, else ABN_ERR_INVALID_ARG), what
 * abn_pairwise_divergence_packed_dev reads (src/pedigree.rs:210-261); nothing of per-site size reaches the host.
 * kernel_ms (may be NULL): the kernel's HIP-event time.  Returns after the work has completed. */
int abn_sim_codes_dev(abn_ctx* ctx, uint64_t seed, int32_t n_nodes, const int32_t* parent, const uint64_t* thr,
                      const uint8_t* emit, int64_t n_sites, void* dev_packed, int64_t row_stride_bytes, double* kernel_ms);
/* Pedigree::build (src/pedigree.rs:92-193) of simulated methylomes: the simulation into a device matrix, DMatrix::from by
 * abn_pairwise_divergence_packed_dev, and the rows of DMatrix::convert (:281-333) — rows double [pairs x 4] = (t0, t1, t2,
 * D) for the pairs i < j of the emitted nodes in node order, t0 the generation of the pair's last common ancestor.  *p0uu
 * (:171-183): a site's level is state / 2, rc_meth_lvl of a sample (double)(n1 + 2 n2) / (2.0 (double)n_sites) from the
 * sums of abn_pairwise_transitions_packed_dev's table, p0uu the mean of 1 - rc_meth_lvl summed in sample order.  ms2 (may be
 * NULL): the HIP-event times of the simulation and of the two passes over the matrix behind it (the divergence scan and the
 * transition table, summed).  ABN_ERR_INVALID_ARG: as abn_sim_codes; a null generation,
 * rows or p0uu; n_sites < 1; fewer than two emitted nodes. */
int abn_sim_pedigree(abn_ctx* ctx, uint64_t seed, int32_t n_nodes, const int32_t* parent, const int32_t* generation,
                     const uint64_t* thr, const uint8_t* emit, int64_t n_sites, double* rows, double* p0uu, double* ms2);

/* ------------------------------------------------------------------ the observation step and replicate studies
 * What a caller of methylation states sees of a true state: another state (a miscall) or nothing — a call below the
 * posterior filter, which the reference drops per pair (src/pedigree.rs:249-251) and leaves out of rc_meth_lvl
 * (src/pedigree.rs:159-175).  othr uint64 [3][3], each row non-decreasing.  For the row of node v, site k, true state s in
 * {0, 1, 2}: the draw w(k, v) is built exactly as u(k, v) above with c3 = 6 (kTagObs = 6u); c2 = v is the NODE's index, not
 * the row's.  The observed field is (w >= othr[s][0]) + (w >= othr[s][1]) + (w >= othr[s][2]); the field 3 is "filtered".
 * An input field that already is 3 stays 3; the fields from n_sites to the end of abn_packed_row_stride(n_sites) bytes are
 * written as 3; bytes beyond abn_packed_row_stride(n_sites) of a row are neither read nor written.
 *
 * abn_sim_obs_thresholds (host arithmetic, no device): othr from miscall[3][3] (row s: the probabilities that a kept call of
 * a true state s reads 0, 1, 2) and dropout[3] (the probability that a call of a true state s is filtered).  With q = 1 -
 * dropout[s]: c0 = q m[s][0], c1 = q (m[s][0] + m[s][1]), c2 = q, each through threshold(c) of abn_sim_thresholds, then
 * t1 = max(t1, t0), t2 = max(t2, t1).  ABN_ERR_INVALID_ARG with `text`: null pointers, a value outside [0, 1] or not
 * finite, a miscall row whose sum differs from 1 by more than 1e-12. */
int abn_sim_obs_thresholds(const double miscall[9], const double dropout[3], uint64_t othr[9], char* text, int32_t text_bytes);
/* The observation of the HOST matrix packed_in [n_rows x in_stride] into packed_out [n_rows x out_stride]; row r belongs to
 * node node_of_row[r].  packed_in == packed_out with equal strides is allowed, any other overlap refused.
 * ABN_ERR_INVALID_ARG with a text, before any launch: null pointers, n_rows < 1 or > 65535, a node_of_row outside 0..65534,
 * a decreasing othr row, n_sites < 0 or > 2^34, a stride that is not a multiple of 64 or is below
 * abn_packed_row_stride(n_sites).  n_sites == 0: ABN_OK, nothing written. */
int abn_sim_observe(abn_ctx* ctx, uint64_t seed, int32_t n_rows, const int32_t* node_of_row, const uint64_t* othr,
                    int64_t n_sites, const uint8_t* packed_in, int64_t in_stride, uint8_t* packed_out, int64_t out_stride);
/* ... on DEVICE matrices (both 16-byte aligned, else ABN_ERR_INVALID_ARG); kernel_ms (may be NULL): the kernel's HIP-event
 * time.  Returns after the work has completed. */
int abn_sim_observe_dev(abn_ctx* ctx, uint64_t seed, int32_t n_rows, const int32_t* node_of_row, const uint64_t* othr,
                        int64_t n_sites, const void* dev_in, int64_t in_stride, void* dev_out, int64_t out_stride,
                        double* kernel_ms);
/* A replicate study: replicate r is the sites [r L, (r + 1) L) of ONE simulation of R L sites (L = n_sites, R =
 * n_replicates), so its codes are those columns of abn_sim_codes(.., R L).  The chain: the simulation into a device matrix,
 * the observation in place where othr is given (NULL: no observation step), abn_pairwise_divergence_windows_packed_dev and
 * abn_packed_census_windows_dev over the R ranges; only the results reach the host.  times double [pairs x 3] = (t0, t1, t2)
 * of DMatrix::convert (src/pedigree.rs:281-333) as abn_sim_pedigree forms them; dvalue double [R x pairs]; p0uu double [R]:
 * the mean, in sample order, of 1 - (double)(n1 + 2 n2) / (2.0 (double)(n0 + n1 + n2)) over a sample's kept sites
 * (src/pedigree.rs:159-183) — a sample that keeps nothing gives the reference's 0 / 0, NaN, which is passed on; census uint64
 * [R x emitted x 3] (may be NULL); ms4 (may be NULL): the HIP-event times of the simulation, the observation, the scan and the
 * census.  With R = 1 and othr = NULL, times / dvalue / p0uu are abn_sim_pedigree's bits.  ABN_ERR_INVALID_ARG: as
 * abn_sim_codes; a null generation, times, dvalue or p0uu; L < 1; R < 1; R L > 2^34; fewer than two emitted nodes; a
 * decreasing othr row. */
int abn_sim_study(abn_ctx* ctx, uint64_t seed, int32_t n_nodes, const int32_t* parent, const int32_t* generation,
                  const uint64_t* thr, const uint8_t* emit, const uint64_t* othr, int64_t n_sites, int32_t n_replicates,
                  double* times, double* dvalue, double* p0uu, uint64_t* census, double* ms4);

#ifdef __cplusplus
}
#endif
#endif /* ABNEUTRAL_H */
