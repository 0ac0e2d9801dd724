// Pedigree construction: the four pairwise divergence scans abn_pairwise_divergence* — byte codes
// or 2-bit packed codes, the whole matrix or many windows of it — each with a host entry and a _dev entry — and the
// state transition tables abn_pairwise_transitions* of the packed two (abn_pairwise_transitions.hpp), and the state census of
// a packed matrix per column range abn_packed_census_windows* (abn_packed_census.hpp).
// The scan kernels are in abn_pairwise_mx.hpp, abn_pairwise_packed.hpp, abn_pairwise_windows.hpp and
// abn_pairwise_windows_packed.hpp; the fit path (abn_api.hip, abn_context.hip, abn_plan.hip) does not include them.
#define ABN_TRANSITIONS_KERNELS
#define ABN_CENSUS_KERNELS
#include "abn_host.hpp"
#include "abn_packed_census.hpp"
#include "abn_pairwise_mx.hpp"
#include "abn_pairwise_packed.hpp"
#include "abn_pairwise_transitions.hpp"
#include "abn_pairwise_windows.hpp"
#include "abn_pairwise_windows_packed.hpp"

using namespace abn;

// ------------------------------------------------------------------------------------------------
// pedigree construction: pairwise divergence (src/pedigree.rs:210-261)
// ------------------------------------------------------------------------------------------------
// Exact integer Gram products on the matrix pipe (abn_pairwise_mx.hpp): any number of samples, the sample axis tiled in
// groups of 64; codes already on the device, outputs on the device (any may be null).
constexpr long long kPmxMaxJobs = 8192;  // jobs per launch: 32 KiB of packed sums each (256 MiB of `partial`)

// The scan kernels by format: Family::kernel<NB, DIAG>.
template <bool AL4>
struct Mx {
  template <int NB, bool DIAG>
  static constexpr auto kernel = abn_pairwise_mx_kernel<NB, DIAG, AL4>;
};
struct Packed {
  template <int NB, bool DIAG>
  static constexpr auto kernel = abn_pairwise_packed_kernel<NB, DIAG>;
};
template <bool AL4>
struct Win {
  template <int NB, bool DIAG>
  static constexpr auto kernel = abn_pairwise_win_kernel<NB, DIAG, AL4>;
};
struct WinPacked {
  template <int NB, bool DIAG>
  static constexpr auto kernel = abn_pairwise_win_packed_kernel<NB, DIAG>;
};
struct Trans {
  template <int NB, bool DIAG>
  static constexpr auto kernel = abn_pairwise_trans_kernel<NB, DIAG>;
};

// `grid` jobs of one family of super-pairs: the pairs R < C are 4 x 4 blocks of 16 samples, a diagonal super-pair has nb
template <class Family, class Args>
static hipError_t launch_scan(int nb, bool diag, unsigned grid, hipStream_t s, const Args& a) {
  auto launch = [&](auto kernel) { hipLaunchKernelGGL(kernel, dim3(grid), dim3(kPmxThreads), 0, s, a); };
  if (!diag) {
    launch(Family::template kernel<4, false>);
  } else {
    switch (nb) {
      case 1: launch(Family::template kernel<1, true>); break;
      case 2: launch(Family::template kernel<2, true>); break;
      case 3: launch(Family::template kernel<3, true>); break;
      default: launch(Family::template kernel<4, true>); break;
    }
  }
  return hipGetLastError();
}

// groups of 64 samples; nb: the blocks of 16 samples of a diagonal super-pair's kernel (those that exist in a lone group)
static int pairwise_groups(int n, int& nb) {
  const int ngroups = (n + 63) / 64;
  nb = ngroups == 1 ? (n + 15) / 16 : 4;
  return ngroups;
}

// the codes of a host entry on the device (at least min_bytes: the loaders' spare bytes)
static int upload_codes(abn_ctx* c, DevBuf<uint8_t>& d, const uint8_t* codes, size_t bytes, size_t min_bytes) {
  HIPCHK(c, d.alloc(std::max(bytes, min_bytes)));
  if (bytes > 0) HIPCHK(c, hipMemcpyAsync(d.p, codes, bytes, hipMemcpyHostToDevice, c->stream));
  return ABN_OK;
}

// One family of super-pairs (the ngroups diagonal ones, or the pairs R < C), in slabs of at most kPmxMaxJobs jobs: each
// slab is a scan launch and a reduce launch that writes its pairs of the result.  Args: PairMxArgs or PairPackedArgs;
// `steps`: the 64-byte steps of a row (64 sites of byte codes, 256 of packed ones); launch(diag, grid, args).
template <class Args, class Launch>
static int pairwise_family(abn_ctx* c, Args a, long long steps, long long L, bool diag, long long nsp, long long cu_jobs,
                           DevBuf<unsigned long long>& partial, unsigned long long* ddiff, unsigned long long* dboth,
                           double* ddval, Launch launch) {
  if (nsp <= 0) return ABN_OK;
  // chunks per super-pair: enough jobs to fill the GPU (cu_jobs workgroups per CU), every wavefront at least a few
  // steps (64 bytes of every row each), and no chunk beyond 2^30 sites (the packed 32-bit halves of a job's sums)
  long long nchunks = std::max<long long>(1, ((long long)c->cus * cu_jobs + nsp - 1) / nsp);
  nchunks = std::min<long long>(nchunks, std::max<long long>(1, steps / (4 * kPmxWaves)));
  nchunks = std::max<long long>(nchunks, (L >> 30) + 1);
  if (L == 0) nchunks = 1;
  a.nchunks = (int)nchunks;
  const long long slab = std::max<long long>(1, kPmxMaxJobs / nchunks);
  HIPCHK(c, partial.alloc((size_t)std::min(slab, nsp) * (size_t)nchunks * kPmxJobElems));
  a.partial = partial.p;
  for (long long s0 = 0; s0 < nsp; s0 += slab) {
    const long long ns = std::min(slab, nsp - s0);
    a.first = s0;
    if (L > 0) HIPCHK(c, launch(diag, (unsigned)(ns * nchunks), a));
    // (no sites: zero rows are summed and every pair is 0 / 0)
    hipLaunchKernelGGL(abn_pairwise_reduce_tiles_kernel, dim3((unsigned)(ns * 256)), dim3(16 * kPmxReduceGroups), 0,
                       c->stream, partial.p, L > 0 ? (int)nchunks : 0, a.n, a.ngroups, diag ? 1 : 0, s0, ddiff, dboth,
                       ddval);
    HIPCHK(c, hipGetLastError());
  }
  return ABN_OK;
}

// Both families of a scan between the two events of kernel_ms.  row_bytes: what the scan reads of every row.
template <class Args, class Launch>
static int pairwise_scan_on_device(abn_ctx* c, const Args& a, long long steps, long long L, long long row_bytes,
                                   unsigned long long* ddiff, unsigned long long* dboth, double* ddval,
                                   double* kernel_ms, Launch launch) {
  DevBuf<unsigned long long> pdiag, poff;
  EventPair ev;
  if (int rc = ev.begin(c, kernel_ms != nullptr)) return rc;
  // workgroups per CU: two (eight wavefronts streaming per CU) once the scan is long enough to pay for twice the partial
  // rows; one below (byte codes, 50 x 2 M sites: 28.6 against 30.5 us; 50 x 32 M: 304 against 282 us)
  long long cu_diag = (long long)a.n * row_bytes >= (256ll << 20) ? 2 : 1, cu_off = 1;
#ifdef ABN_MEASUREMENT_KNOBS
  if (const char* e = getenv("ABN_PMX_CU_JOBS")) cu_diag = cu_off = std::max(1, atoi(e));
#endif
  const long long g = a.ngroups;
  int rc = pairwise_family(c, a, steps, L, true, g, cu_diag, pdiag, ddiff, dboth, ddval, launch);
  if (!rc) rc = pairwise_family(c, a, steps, L, false, g * (g - 1) / 2, cu_off, poff, ddiff, dboth, ddval, launch);
  if (!rc) rc = ev.end(c, kernel_ms);
  if (rc) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));  // the partial rows are freed on return
  return ABN_OK;
}

static int pairwise_mx_on_device(abn_ctx* c, const uint8_t* dcodes, int n, long long L, unsigned long long* ddiff,
                                 unsigned long long* dboth, double* ddval, double* kernel_ms) {
  if (n > 65535) return set_err(c, ABN_ERR_INVALID_ARG, "too many samples");
  PairMxArgs a{};
  a.codes = dcodes;
  a.n = n;
  a.L = L;
  int nb;
  a.ngroups = pairwise_groups(n, nb);
  const bool al4 = (L % 4 == 0) && ((uintptr_t)dcodes % 4 == 0);
  return pairwise_scan_on_device(c, a, (L + 63) / 64, L, L, ddiff, dboth, ddval, kernel_ms,
                                 [&](bool diag, unsigned grid, const PairMxArgs& args) {
                                   return al4 ? launch_scan<Mx<true>>(nb, diag, grid, c->stream, args)
                                              : launch_scan<Mx<false>>(nb, diag, grid, c->stream, args);
                                 });
}

extern "C" int abn_pairwise_divergence_dev(abn_ctx* c, const void* dev_codes, int32_t n_samples, int64_t n_sites,
                                           void* dev_diff, void* dev_both, void* dev_dvalue, double* kernel_ms) {
  if (!c) return ABN_ERR_INVALID_ARG;
  if (!dev_codes || n_samples <= 0 || n_sites < 0) return set_err(c, ABN_ERR_INVALID_ARG, "null/size");
  if (n_samples < 2) return ABN_OK;
  HIPCHK(c, hipSetDevice(c->device));
  PoolScope pool_scope(c);
  return pairwise_mx_on_device(c, (const uint8_t*)dev_codes, n_samples, n_sites, (unsigned long long*)dev_diff,
                            (unsigned long long*)dev_both, (double*)dev_dvalue, kernel_ms);
}

extern "C" int abn_pairwise_divergence(abn_ctx* c, const uint8_t* codes, int32_t n_samples, int64_t n_sites,
                                       uint64_t* diff, uint64_t* both, double* dvalue) {
  if (!c) return ABN_ERR_INVALID_ARG;
  if (!codes || n_samples <= 0 || n_sites < 0) return set_err(c, ABN_ERR_INVALID_ARG, "null/size");
  const size_t n = (size_t)n_samples, npairs = n * (n - 1) / 2;
  if (npairs == 0) return ABN_OK;
  HIPCHK(c, hipSetDevice(c->device));
  PoolScope pool_scope(c);
  DevBuf<uint8_t> dcodes;
  if (int rc = upload_codes(c, dcodes, codes, n * (size_t)n_sites, 4)) return rc;
  return pairwise_to_host(c, npairs, diff, both, dvalue, [&](auto* dd, auto* db, auto* dv) {
    return pairwise_mx_on_device(c, dcodes.p, n_samples, n_sites, dd, db, dv, nullptr);
  });
}

// ------------------------------------------------------------------------------------------------
// the same on 2-bit packed codes (src/pedigree.rs:210-261; format: include/abneutral.h, abn_pack_codes)
// ------------------------------------------------------------------------------------------------
static int pairwise_packed_check(abn_ctx* c, const void* packed, int32_t n, int64_t L, int64_t stride) {
  if (!packed || n <= 0 || L < 0) return set_err(c, ABN_ERR_INVALID_ARG, "null/size");
  if (stride < 0 || stride % 64 != 0 || stride < abn_packed_row_stride(L))
    return set_err(c, ABN_ERR_INVALID_ARG, "row_stride_bytes is not a multiple of 64 that holds n_sites fields");
  if (n > 65535) return set_err(c, ABN_ERR_INVALID_ARG, "too many samples");
  return ABN_OK;
}

static int pairwise_packed_on_device(abn_ctx* c, const uint8_t* dpacked, int n, long long L, long long stride,
                                     unsigned long long* ddiff, unsigned long long* dboth, double* ddval,
                                     double* kernel_ms) {
  PairPackedArgs a{};
  a.packed = dpacked;
  a.row_stride = stride;
  a.nk = (L + 255) / 256;
  a.n = n;
  int nb;
  a.ngroups = pairwise_groups(n, nb);
  // a chunk is a whole number of 64-byte super-steps of every row; the chunk rule is the byte scan's in those steps (a
  // wavefront's floor of four is then 16 matrix steps): the launch fills the GPU from a quarter of the bytes on
  return pairwise_scan_on_device(c, a, a.nk, L, 64 * a.nk, ddiff, dboth, ddval, kernel_ms,
                                 [&](bool diag, unsigned grid, const PairPackedArgs& args) {
                                   return launch_scan<Packed>(nb, diag, grid, c->stream, args);
                                 });
}

extern "C" int abn_pairwise_divergence_packed_dev(abn_ctx* c, const void* dev_packed, int32_t n_samples, int64_t n_sites,
                                                  int64_t row_stride_bytes, void* dev_diff, void* dev_both,
                                                  void* dev_dvalue, double* kernel_ms) {
  if (!c) return ABN_ERR_INVALID_ARG;
  if (int rc = pairwise_packed_check(c, dev_packed, n_samples, n_sites, row_stride_bytes)) return rc;
  if ((uintptr_t)dev_packed % 16 != 0) return set_err(c, ABN_ERR_INVALID_ARG, "dev_packed is not 16-byte aligned");
  if (n_samples < 2) return ABN_OK;
  HIPCHK(c, hipSetDevice(c->device));
  PoolScope pool_scope(c);
  return pairwise_packed_on_device(c, (const uint8_t*)dev_packed, n_samples, n_sites, row_stride_bytes,
                                   (unsigned long long*)dev_diff, (unsigned long long*)dev_both, (double*)dev_dvalue,
                                   kernel_ms);
}

extern "C" int abn_pairwise_divergence_packed(abn_ctx* c, const uint8_t* packed, int32_t n_samples, int64_t n_sites,
                                              int64_t row_stride_bytes, uint64_t* diff, uint64_t* both, double* dvalue) {
  if (!c) return ABN_ERR_INVALID_ARG;
  if (int rc = pairwise_packed_check(c, packed, n_samples, n_sites, row_stride_bytes)) return rc;
  const size_t n = (size_t)n_samples, npairs = n * (n - 1) / 2;
  if (npairs == 0) return ABN_OK;
  HIPCHK(c, hipSetDevice(c->device));
  PoolScope pool_scope(c);
  DevBuf<uint8_t> dpacked;  // (device allocations are aligned far beyond the 16 bytes the kernel asks for)
  if (int rc = upload_codes(c, dpacked, packed, n * (size_t)row_stride_bytes, 64)) return rc;
  return pairwise_to_host(c, npairs, diff, both, dvalue, [&](auto* dd, auto* db, auto* dv) {
    return pairwise_packed_on_device(c, dpacked.p, n_samples, n_sites, row_stride_bytes, dd, db, dv, nullptr);
  });
}

// ------------------------------------------------------------------------------------------------
// the same for many windows of one code matrix (src/cli/metaprofile.rs:50-72 around src/pedigree.rs:210-261)
// ------------------------------------------------------------------------------------------------
// The jobs of one family of super-pairs over all windows, in launches ("slabs") of at most kPmxMaxJobs jobs; the chunks
// of one (window, super-pair) never straddle two slabs, so a slab's reduce launch finds all rows of its tasks.
// A window's chunks are cut at multiples of chunk[w] from its begin rounded down to `align` sites (1: byte codes, from the
// begin itself; 256: packed codes, whole super-steps); launch(diag, jobs, args) starts the scan kernel of the format and
// reduce(diag, tasks, ntasks, args) the kernel that sums a slab's partial rows.  row_words and max_jobs: the 64-bit
// words of a partial row and the jobs per launch of the scan (the divergence scans' unless set before plan).
struct PairWinFamily {
  struct Slab { size_t job0, njobs, task0, ntasks, nrows; };
  size_t row_words = kPmxJobElems;
  long long max_jobs = kPmxMaxJobs;
  std::vector<PairWinJob> jobs;
  std::vector<PairWinTask> tasks;
  std::vector<Slab> slabs;
  size_t max_rows = 0;
  DevBuf<PairWinJob> djobs;
  DevBuf<PairWinTask> dtasks;
  DevBuf<unsigned long long> partial;

  void plan(long long nsp, const int64_t* begin, const int64_t* end, int W, const std::vector<long long>& chunk,
            long long align) {
    if (nsp <= 0) return;
    Slab cur{0, 0, 0, 0, 0};
    for (int w = 0; w < W; ++w) {
      const long long b0 = begin[w] - begin[w] % align;
      const long long nch = std::max<long long>(1, (end[w] - b0 + chunk[w] - 1) / chunk[w]);
      for (long long sp = 0; sp < nsp; ++sp) {
        if (cur.njobs + (size_t)nch > (size_t)max_jobs) {
          slabs.push_back(cur);
          cur = Slab{jobs.size(), 0, tasks.size(), 0, 0};
        }
        if (nch > 1) {
          tasks.push_back(PairWinTask{w, (int)sp, (int)cur.nrows, (int)nch, 0});
          ++cur.ntasks;
        }
        for (long long k = 0; k < nch; ++k) {
          const long long b = b0 + k * chunk[w];
          jobs.push_back(PairWinJob{std::max<long long>(b, begin[w]), std::min<long long>(b + chunk[w], end[w]), w, (int)sp,
                                    nch > 1 ? (int)cur.nrows++ : -1});
        }
        cur.njobs += (size_t)nch;
      }
    }
    slabs.push_back(cur);
    for (const Slab& s : slabs) max_rows = std::max(max_rows, s.nrows);
  }
  int upload(abn_ctx* c) {
    HIPCHK(c, djobs.alloc(jobs.size()));
    HIPCHK(c, dtasks.alloc(tasks.size()));
    HIPCHK(c, partial.alloc(max_rows * row_words));
    if (!jobs.empty())
      HIPCHK(c, hipMemcpyAsync(djobs.p, jobs.data(), djobs.bytes(), hipMemcpyHostToDevice, c->stream));
    if (!tasks.empty())
      HIPCHK(c, hipMemcpyAsync(dtasks.p, tasks.data(), dtasks.bytes(), hipMemcpyHostToDevice, c->stream));
    return ABN_OK;
  }
  template <class Args, class Launch, class Reduce>
  int run(abn_ctx* c, Args a, bool diag, Launch launch, Reduce reduce) {
    a.partial = reinterpret_cast<decltype(a.partial)>(partial.p);
    for (const Slab& s : slabs) {
      if (s.njobs == 0) continue;
      a.jobs = djobs.p + s.job0;
      HIPCHK(c, launch(diag, (unsigned)s.njobs, a));
      if (s.ntasks == 0) continue;
      reduce(diag, dtasks.p + s.task0, (unsigned)s.ntasks, a);
      HIPCHK(c, hipGetLastError());
    }
    return ABN_OK;
  }
};

// Both families of a windows scan between the two events of kernel_ms: plan, upload the job tables, run.
template <class Args, class Launch, class Reduce>
static int pairwise_windows_run(abn_ctx* c, const Args& a, const int64_t* begin, const int64_t* end, int W,
                                const std::vector<long long>& chunk, long long align, double* kernel_ms, Launch launch,
                                Reduce reduce, size_t row_words = kPmxJobElems, long long max_jobs = kPmxMaxJobs) {
  const long long g = a.ngroups;
  PairWinFamily fdiag, foff;  // (their host tables outlive the copies: the stream is synchronised below)
  fdiag.row_words = foff.row_words = row_words;
  fdiag.max_jobs = foff.max_jobs = max_jobs;
  fdiag.plan(g, begin, end, W, chunk, align);
  foff.plan(g * (g - 1) / 2, begin, end, W, chunk, align);
  int rc = fdiag.upload(c);
  if (!rc) rc = foff.upload(c);
  if (rc) return rc;
  EventPair ev;
  if ((rc = ev.begin(c, kernel_ms != nullptr))) return rc;
  rc = fdiag.run(c, a, true, launch, reduce);
  if (!rc) rc = foff.run(c, a, false, launch, reduce);
  if (!rc) rc = ev.end(c, kernel_ms);
  if (rc) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));  // the job tables and the partial rows are freed on return
  return ABN_OK;
}

// every window is a column range of rows of `limit` sites (byte codes: row_stride; packed codes: n_sites)
static int pairwise_windows_in_rows(abn_ctx* c, const int64_t* begin, const int64_t* end, int W, int64_t limit) {
  for (int w = 0; w < W; ++w)
    if (begin[w] < 0 || begin[w] > end[w] || end[w] > limit)
      return set_err(c, ABN_ERR_INVALID_ARG, "window " + std::to_string(w) + " is not a column range of the rows");
  return ABN_OK;
}

// Sites per job of each window: `sites` (kPmxWinChunkSites, kPmxWinPackedChunkSites), more — whole line pairs of a row and
// whole steps of `align` sites — only where a window would otherwise need more rows of `partial` than one launch keeps.
// Counted from the window's begin rounded down to `align` sites (1: byte codes; kPackedStepSites: packed codes).
// max_jobs: the jobs of one launch (PairWinFamily::max_jobs).
static int pairwise_windows_chunks(abn_ctx* c, const int64_t* begin, const int64_t* end, int W, long long sites,
                                   long long align, std::vector<long long>& chunk, long long max_jobs = kPmxMaxJobs) {
  const long long unit = std::max<long long>(align, 128);
  chunk.resize((size_t)W);
  for (int w = 0; w < W; ++w) {
    const long long span = end[w] - (begin[w] - begin[w] % align);
    long long ch = sites;
    if ((span + ch - 1) / ch > max_jobs) ch = ((span + max_jobs - 1) / max_jobs + unit - 1) / unit * unit;
    if (ch >= (1ll << 30)) return set_err(c, ABN_ERR_INVALID_ARG, "window too long");
    chunk[(size_t)w] = ch;
  }
  return ABN_OK;
}

// the reduce launch of both divergence windows scans
static void pairwise_win_reduce(abn_ctx* c, bool diag, const PairWinTask* tasks, unsigned ntasks, const PairWinArgs& a) {
  hipLaunchKernelGGL(abn_pairwise_win_reduce_kernel, dim3(ntasks * 256), dim3(16 * kPmxReduceGroups), 0, c->stream,
                     a.partial, tasks, a.n, a.ngroups, diag ? 1 : 0, a.diff, a.both, a.dvalue);
}

// the arguments of both windows scans; nb as pairwise_groups
static PairWinArgs pairwise_win_args(const uint8_t* dcodes, long long row_stride, int n, unsigned long long* ddiff,
                                     unsigned long long* dboth, double* ddval, int& nb) {
  PairWinArgs a{};
  a.codes = dcodes;
  a.row_stride = row_stride;
  a.n = n;
  a.ngroups = pairwise_groups(n, nb);
  a.diff = ddiff;
  a.both = dboth;
  a.dvalue = ddval;
  return a;
}

static int pairwise_windows_check(abn_ctx* c, const void* codes, int32_t n, int64_t row_stride, const int64_t* begin,
                                  const int64_t* end, int32_t W, std::vector<long long>& chunk) {
  if (!codes || n <= 0 || row_stride < 0 || W < 0 || (W > 0 && (!begin || !end)))
    return set_err(c, ABN_ERR_INVALID_ARG, "null/size");
  if (n > 65535) return set_err(c, ABN_ERR_INVALID_ARG, "too many samples");
  if (int rc = pairwise_windows_in_rows(c, begin, end, W, row_stride)) return rc;
  return pairwise_windows_chunks(c, begin, end, W, kPmxWinChunkSites, 1, chunk);
}

static int pairwise_windows_on_device(abn_ctx* c, const uint8_t* dcodes, int n, long long row_stride,
                                      const int64_t* begin, const int64_t* end, int W,
                                      const std::vector<long long>& chunk, unsigned long long* ddiff,
                                      unsigned long long* dboth, double* ddval, double* kernel_ms) {
  int nb;
  const PairWinArgs a = pairwise_win_args(dcodes, row_stride, n, ddiff, dboth, ddval, nb);
  bool al4 = (row_stride % 4 == 0) && ((uintptr_t)dcodes % 4 == 0);
  for (int w = 0; w < W; ++w) al4 = al4 && begin[w] % 4 == 0;
  return pairwise_windows_run(c, a, begin, end, W, chunk, 1, kernel_ms,
                              [&](bool diag, unsigned grid, const PairWinArgs& args) {
                                return al4 ? launch_scan<Win<true>>(nb, diag, grid, c->stream, args)
                                           : launch_scan<Win<false>>(nb, diag, grid, c->stream, args);
                              },
                              [&](bool diag, const PairWinTask* tasks, unsigned ntasks, const PairWinArgs& args) {
                                pairwise_win_reduce(c, diag, tasks, ntasks, args);
                              });
}

extern "C" int abn_pairwise_divergence_windows_dev(abn_ctx* c, const void* dev_codes, int32_t n_samples,
                                                   int64_t row_stride, const int64_t* site_begin,
                                                   const int64_t* site_end, int32_t n_windows, void* dev_diff,
                                                   void* dev_both, void* dev_dvalue, double* kernel_ms) {
  if (!c) return ABN_ERR_INVALID_ARG;
  std::vector<long long> chunk;
  if (int rc = pairwise_windows_check(c, dev_codes, n_samples, row_stride, site_begin, site_end, n_windows, chunk))
    return rc;
  if (n_samples < 2 || n_windows == 0) return ABN_OK;
  HIPCHK(c, hipSetDevice(c->device));
  PoolScope pool_scope(c);
  return pairwise_windows_on_device(c, (const uint8_t*)dev_codes, n_samples, row_stride, site_begin, site_end, n_windows,
                                    chunk, (unsigned long long*)dev_diff, (unsigned long long*)dev_both,
                                    (double*)dev_dvalue, kernel_ms);
}

extern "C" int abn_pairwise_divergence_windows(abn_ctx* c, const uint8_t* codes, int32_t n_samples, int64_t row_stride,
                                               const int64_t* site_begin, const int64_t* site_end, int32_t n_windows,
                                               uint64_t* diff, uint64_t* both, double* dvalue) {
  if (!c) return ABN_ERR_INVALID_ARG;
  std::vector<long long> chunk;
  if (int rc = pairwise_windows_check(c, codes, n_samples, row_stride, site_begin, site_end, n_windows, chunk)) return rc;
  if (n_samples < 2 || n_windows == 0) return ABN_OK;
  const size_t n = (size_t)n_samples, nout = n * (n - 1) / 2 * (size_t)n_windows;
  HIPCHK(c, hipSetDevice(c->device));
  PoolScope pool_scope(c);
  DevBuf<uint8_t> dcodes;
  if (int rc = upload_codes(c, dcodes, codes, n * (size_t)row_stride, 4)) return rc;
  return pairwise_to_host(c, nout, diff, both, dvalue, [&](auto* dd, auto* db, auto* dv) {
    return pairwise_windows_on_device(c, dcodes.p, n_samples, row_stride, site_begin, site_end, n_windows, chunk, dd, db,
                                      dv, nullptr);
  });
}

// ------------------------------------------------------------------------------------------------
// ... and for many windows of one 2-bit packed matrix (src/cli/metaprofile.rs:50-72 around src/pedigree.rs:210-261)
// ------------------------------------------------------------------------------------------------
static int pairwise_windows_packed_check(abn_ctx* c, const void* packed, int32_t n, int64_t L, int64_t stride,
                                         const int64_t* begin, const int64_t* end, int32_t W,
                                         std::vector<long long>& chunk, long long max_jobs = kPmxMaxJobs) {
  if (int rc = pairwise_packed_check(c, packed, n, L, stride)) return rc;
  if (W < 0 || (W > 0 && (!begin || !end))) return set_err(c, ABN_ERR_INVALID_ARG, "null/size");
  if (int rc = pairwise_windows_in_rows(c, begin, end, W, L)) return rc;
  return pairwise_windows_chunks(c, begin, end, W, kPmxWinPackedChunkSites, kPackedStepSites, chunk, max_jobs);
}

static int pairwise_windows_packed_on_device(abn_ctx* c, const uint8_t* dpacked, int n, long long stride,
                                             const int64_t* begin, const int64_t* end, int W,
                                             const std::vector<long long>& chunk, unsigned long long* ddiff,
                                             unsigned long long* dboth, double* ddval, double* kernel_ms) {
  int nb;
  const PairWinArgs a = pairwise_win_args(dpacked, stride, n, ddiff, dboth, ddval, nb);
  return pairwise_windows_run(c, a, begin, end, W, chunk, kPackedStepSites, kernel_ms,
                              [&](bool diag, unsigned grid, const PairWinArgs& args) {
                                return launch_scan<WinPacked>(nb, diag, grid, c->stream, args);
                              },
                              [&](bool diag, const PairWinTask* tasks, unsigned ntasks, const PairWinArgs& args) {
                                pairwise_win_reduce(c, diag, tasks, ntasks, args);
                              });
}

int abn::pairwise_windows_packed_dev(abn_ctx* c, const void* dev_packed, int32_t n_samples, int64_t n_sites,
                                     int64_t row_stride_bytes, const int64_t* site_begin, const int64_t* site_end,
                                     int32_t n_windows, void* dev_diff, void* dev_both, void* dev_dvalue,
                                     double* kernel_ms) {
  std::vector<long long> chunk;
  if (int rc = pairwise_windows_packed_check(c, dev_packed, n_samples, n_sites, row_stride_bytes, site_begin, site_end,
                                             n_windows, chunk))
    return rc;
  if ((uintptr_t)dev_packed % 16 != 0) return set_err(c, ABN_ERR_INVALID_ARG, "dev_packed is not 16-byte aligned");
  if (n_samples < 2 || n_windows == 0) return ABN_OK;
  HIPCHK(c, hipSetDevice(c->device));
  PoolScope pool_scope(c);
  return pairwise_windows_packed_on_device(c, (const uint8_t*)dev_packed, n_samples, row_stride_bytes, site_begin,
                                           site_end, n_windows, chunk, (unsigned long long*)dev_diff,
                                           (unsigned long long*)dev_both, (double*)dev_dvalue, kernel_ms);
}

extern "C" int abn_pairwise_divergence_windows_packed_dev(abn_ctx* c, const void* dev_packed, int32_t n_samples,
                                                          int64_t n_sites, int64_t row_stride_bytes,
                                                          const int64_t* site_begin, const int64_t* site_end,
                                                          int32_t n_windows, void* dev_diff, void* dev_both,
                                                          void* dev_dvalue, double* kernel_ms) {
  if (!c) return ABN_ERR_INVALID_ARG;
  return pairwise_windows_packed_dev(c, dev_packed, n_samples, n_sites, row_stride_bytes, site_begin, site_end, n_windows,
                                     dev_diff, dev_both, dev_dvalue, kernel_ms);
}

extern "C" int abn_pairwise_divergence_windows_packed(abn_ctx* c, const uint8_t* packed, int32_t n_samples,
                                                      int64_t n_sites, int64_t row_stride_bytes,
                                                      const int64_t* site_begin, const int64_t* site_end,
                                                      int32_t n_windows, uint64_t* diff, uint64_t* both,
                                                      double* dvalue) {
  if (!c) return ABN_ERR_INVALID_ARG;
  std::vector<long long> chunk;
  if (int rc = pairwise_windows_packed_check(c, packed, n_samples, n_sites, row_stride_bytes, site_begin, site_end,
                                             n_windows, chunk))
    return rc;
  if (n_samples < 2 || n_windows == 0) return ABN_OK;
  const size_t n = (size_t)n_samples, nout = n * (n - 1) / 2 * (size_t)n_windows;
  HIPCHK(c, hipSetDevice(c->device));
  PoolScope pool_scope(c);
  DevBuf<uint8_t> dpacked;  // (device allocations are aligned far beyond the 16 bytes the kernel asks for)
  if (int rc = upload_codes(c, dpacked, packed, n * (size_t)row_stride_bytes, 64)) return rc;
  return pairwise_to_host(c, nout, diff, both, dvalue, [&](auto* dd, auto* db, auto* dv) {
    return pairwise_windows_packed_on_device(c, dpacked.p, n_samples, row_stride_bytes, site_begin, site_end, n_windows,
                                             chunk, dd, db, dv, nullptr);
  });
}

// ------------------------------------------------------------------------------------------------
// the 3 x 3 state transition table of every pair (the joint table behind src/pedigree.rs:236-257), whole packed matrix or
// many windows of it: abn_pairwise_transitions.hpp
// ------------------------------------------------------------------------------------------------
// dtable [W][pairs][9] on the device.  A job of the plan is a (window, super-pair, chunk); the grid has one workgroup
// per row block of each.  Every pair of every window is written (an empty window: by its one job that runs no step).
static int transitions_on_device(abn_ctx* c, const uint8_t* dpacked, int n, long long stride, const int64_t* begin,
                                 const int64_t* end, int W, const std::vector<long long>& chunk,
                                 unsigned long long* dtable, double* kernel_ms) {
  PairTransArgs a{};
  a.codes = dpacked;
  a.row_stride = stride;
  a.n = n;
  int nb;
  a.ngroups = pairwise_groups(n, nb);
  a.table = dtable;
  return pairwise_windows_run(
      c, a, begin, end, W, chunk, kPackedStepSites, kernel_ms,
      [&](bool diag, unsigned jobs, const PairTransArgs& args) {
        return launch_scan<Trans>(nb, diag, jobs * (unsigned)(diag ? nb : 4), c->stream, args);
      },
      [&](bool diag, const PairWinTask* tasks, unsigned ntasks, const PairTransArgs& args) {
        hipLaunchKernelGGL(abn_pairwise_trans_reduce_kernel, dim3(ntasks * 256),
                           dim3(kTransReduceRow * kTransReduceGroups), 0, c->stream, args.partial, tasks, args.n,
                           args.ngroups, diag ? 1 : 0, args.table);
      },
      (size_t)kTransRowWords / 2, kTransMaxJobs);
}

int abn::transitions_windows_packed_dev(abn_ctx* c, const void* dev_packed, int32_t n_samples, int64_t n_sites,
                                        int64_t row_stride_bytes, const int64_t* site_begin, const int64_t* site_end,
                                        int32_t n_windows, void* dev_table, double* kernel_ms) {
  std::vector<long long> chunk;
  if (int rc = pairwise_windows_packed_check(c, dev_packed, n_samples, n_sites, row_stride_bytes, site_begin, site_end,
                                             n_windows, chunk, kTransMaxJobs))
    return rc;
  if ((uintptr_t)dev_packed % 16 != 0) return set_err(c, ABN_ERR_INVALID_ARG, "dev_packed is not 16-byte aligned");
  if (n_samples < 2 || n_windows == 0) return ABN_OK;
  if (!dev_table) return set_err(c, ABN_ERR_INVALID_ARG, "null/size");
  HIPCHK(c, hipSetDevice(c->device));
  PoolScope pool_scope(c);
  return transitions_on_device(c, (const uint8_t*)dev_packed, n_samples, row_stride_bytes, site_begin, site_end,
                               n_windows, chunk, (unsigned long long*)dev_table, kernel_ms);
}

int abn::transitions_packed_dev(abn_ctx* c, const void* dev_packed, int32_t n_samples, int64_t n_sites,
                                int64_t row_stride_bytes, void* dev_table, double* kernel_ms) {
  if (int rc = pairwise_packed_check(c, dev_packed, n_samples, n_sites, row_stride_bytes)) return rc;
  const int64_t begin = 0, end = n_sites;  // the whole matrix is one window
  return transitions_windows_packed_dev(c, dev_packed, n_samples, n_sites, row_stride_bytes, &begin, &end, 1, dev_table,
                                        kernel_ms);
}

// the table of a host entry: `count` counts on the device around scan(dtable), then to the host, the stream synchronised
template <class Scan>
static int transitions_to_host(abn_ctx* c, size_t count, uint64_t* table, Scan scan) {
  if (!table) return set_err(c, ABN_ERR_INVALID_ARG, "null/size");
  DevBuf<unsigned long long> dtable;
  HIPCHK(c, dtable.alloc(count));
  if (int rc = scan(dtable.p)) return rc;
  HIPCHK(c, hipMemcpyAsync(table, dtable.p, dtable.bytes(), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return ABN_OK;
}
int abn::transitions_windows_packed_to_host(abn_ctx* c, const void* dev_packed, int32_t n_samples, int64_t n_sites,
                                            int64_t row_stride_bytes, const int64_t* site_begin,
                                            const int64_t* site_end, int32_t n_windows, uint64_t* table) {
  const size_t n = (size_t)n_samples;
  return transitions_to_host(c, n * (n - 1) / 2 * (size_t)n_windows * kTransEntries, table, [&](auto* dt) {
    return transitions_windows_packed_dev(c, dev_packed, n_samples, n_sites, row_stride_bytes, site_begin, site_end,
                                          n_windows, dt, nullptr);
  });
}

extern "C" int abn_pairwise_transitions_packed_dev(abn_ctx* c, const void* dev_packed, int32_t n_samples,
                                                   int64_t n_sites, int64_t row_stride_bytes, void* dev_table,
                                                   double* kernel_ms) {
  if (!c) return ABN_ERR_INVALID_ARG;
  return transitions_packed_dev(c, dev_packed, n_samples, n_sites, row_stride_bytes, dev_table, kernel_ms);
}

extern "C" int abn_pairwise_transitions_windows_packed_dev(abn_ctx* c, const void* dev_packed, int32_t n_samples,
                                                           int64_t n_sites, int64_t row_stride_bytes,
                                                           const int64_t* site_begin, const int64_t* site_end,
                                                           int32_t n_windows, void* dev_table, double* kernel_ms) {
  if (!c) return ABN_ERR_INVALID_ARG;
  return transitions_windows_packed_dev(c, dev_packed, n_samples, n_sites, row_stride_bytes, site_begin, site_end,
                                        n_windows, dev_table, kernel_ms);
}

extern "C" int abn_pairwise_transitions_windows_packed(abn_ctx* c, const uint8_t* packed, int32_t n_samples,
                                                       int64_t n_sites, int64_t row_stride_bytes,
                                                       const int64_t* site_begin, const int64_t* site_end,
                                                       int32_t n_windows, uint64_t* table) {
  if (!c) return ABN_ERR_INVALID_ARG;
  std::vector<long long> chunk;
  if (int rc = pairwise_windows_packed_check(c, packed, n_samples, n_sites, row_stride_bytes, site_begin, site_end,
                                             n_windows, chunk, kTransMaxJobs))
    return rc;
  if (n_samples < 2 || n_windows == 0) return ABN_OK;
  HIPCHK(c, hipSetDevice(c->device));
  PoolScope pool_scope(c);
  DevBuf<uint8_t> dpacked;  // (device allocations are aligned far beyond the 16 bytes the kernel asks for)
  if (int rc = upload_codes(c, dpacked, packed, (size_t)n_samples * (size_t)row_stride_bytes, 64)) return rc;
  return transitions_windows_packed_to_host(c, dpacked.p, n_samples, n_sites, row_stride_bytes, site_begin, site_end,
                                            n_windows, table);
}

extern "C" int abn_pairwise_transitions_packed(abn_ctx* c, const uint8_t* packed, int32_t n_samples, int64_t n_sites,
                                               int64_t row_stride_bytes, uint64_t* table) {
  if (!c) return ABN_ERR_INVALID_ARG;
  if (int rc = pairwise_packed_check(c, packed, n_samples, n_sites, row_stride_bytes)) return rc;
  const int64_t begin = 0, end = n_sites;
  return abn_pairwise_transitions_windows_packed(c, packed, n_samples, n_sites, row_stride_bytes, &begin, &end, 1, table);
}

// ------------------------------------------------------------------------------------------------
// the state census of every sample per column range of a packed matrix (src/pedigree.rs:159-175 over a sample's own kept
// sites): abn_packed_census.hpp
// ------------------------------------------------------------------------------------------------
constexpr long long kCensusSlab = 1ll << 20;  // workgroups on x of one launch

// dcounts [W][n][3] on the device; the cuts of the windows are `chunk`'s, the packed windows scan's
static int census_on_device(abn_ctx* c, const uint8_t* dpacked, int n, long long stride, const int64_t* begin,
                            const int64_t* end, int W, const std::vector<long long>& chunk, unsigned long long* dcounts,
                            double* kernel_ms) {
  std::vector<CensusJob> jobs;
  std::vector<long long> job_off;
  census_plan(begin, end, W, chunk.data(), jobs, job_off);
  const long long J = (long long)jobs.size();
  DevBuf<CensusJob> djobs;
  DevBuf<long long> doff;
  DevBuf<uint32_t> dpartial;
  EventPair ev;
  if (J > 0)
    if (int rc = upload(c, djobs, jobs.data(), (size_t)J)) return rc;
  if (int rc = upload(c, doff, job_off.data(), job_off.size())) return rc;
  HIPCHK(c, dpartial.alloc((size_t)n * (size_t)J * 3));
  if (int rc = ev.begin(c, kernel_ms != nullptr)) return rc;
  for (long long j0 = 0; j0 < J; j0 += kCensusSlab) {
    const unsigned grid = (unsigned)std::min(kCensusSlab, J - j0);
    hipLaunchKernelGGL(abn_packed_census_kernel, dim3(grid, (unsigned)n), dim3(kCensusThreads), 0, c->stream, dpacked, stride,
                       (const CensusJob*)djobs.p, J, j0, dpartial.p);
    HIPCHK(c, hipGetLastError());
  }
  for (long long w0 = 0; w0 < W; w0 += kCensusSlab) {
    const unsigned grid = (unsigned)std::min<long long>(kCensusSlab, W - w0);
    hipLaunchKernelGGL(abn_packed_census_sum_kernel, dim3(grid, (unsigned)n), dim3(kCensusSumThreads), 0, c->stream,
                       (const uint32_t*)dpartial.p, (const long long*)doff.p, J, w0, dcounts);
    HIPCHK(c, hipGetLastError());
  }
  if (int rc = ev.end(c, kernel_ms)) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));  // the host's jobs and offsets stay until the stream has read them
  return ABN_OK;
}

int abn::packed_census_windows_dev(abn_ctx* c, const void* dev_packed, int32_t n_samples, int64_t n_sites,
                                   int64_t row_stride_bytes, const int64_t* site_begin, const int64_t* site_end,
                                   int32_t n_windows, void* dev_counts, double* kernel_ms) {
  std::vector<long long> chunk;
  if (int rc = pairwise_windows_packed_check(c, dev_packed, n_samples, n_sites, row_stride_bytes, site_begin, site_end,
                                             n_windows, chunk))
    return rc;
  if ((uintptr_t)dev_packed % 16 != 0) return set_err(c, ABN_ERR_INVALID_ARG, "dev_packed is not 16-byte aligned");
  if (kernel_ms) *kernel_ms = 0.0;
  if (n_windows == 0) return ABN_OK;
  if (!dev_counts) return set_err(c, ABN_ERR_INVALID_ARG, "null/size");
  try {
    HIPCHK(c, hipSetDevice(c->device));
    PoolScope pool_scope(c);
    return census_on_device(c, (const uint8_t*)dev_packed, n_samples, row_stride_bytes, site_begin, site_end, n_windows, chunk,
                            (unsigned long long*)dev_counts, kernel_ms);
  } catch (const std::bad_alloc&) {
    return set_err(c, ABN_ERR_HIP, "out of host memory");
  }
}

extern "C" int abn_packed_census_windows_dev(abn_ctx* c, const void* dev_packed, int32_t n_samples, int64_t n_sites,
                                             int64_t row_stride_bytes, const int64_t* site_begin, const int64_t* site_end,
                                             int32_t n_windows, void* dev_counts, double* kernel_ms) {
  if (!c) return ABN_ERR_INVALID_ARG;
  return packed_census_windows_dev(c, dev_packed, n_samples, n_sites, row_stride_bytes, site_begin, site_end, n_windows,
                                   dev_counts, kernel_ms);
}

extern "C" int abn_packed_census_windows(abn_ctx* c, const uint8_t* packed, int32_t n_samples, int64_t n_sites,
                                         int64_t row_stride_bytes, const int64_t* site_begin, const int64_t* site_end,
                                         int32_t n_windows, uint64_t* counts) {
  if (!c) return ABN_ERR_INVALID_ARG;
  std::vector<long long> chunk;
  if (int rc = pairwise_windows_packed_check(c, packed, n_samples, n_sites, row_stride_bytes, site_begin, site_end, n_windows,
                                             chunk))
    return rc;
  if (n_windows == 0) return ABN_OK;
  if (!counts) return set_err(c, ABN_ERR_INVALID_ARG, "null/size");
  try {
    HIPCHK(c, hipSetDevice(c->device));
    PoolScope pool_scope(c);
    DevBuf<uint8_t> dpacked;  // (device allocations are aligned far beyond the 16 bytes the kernel asks for)
    DevBuf<unsigned long long> dcounts;
    if (int rc = upload_codes(c, dpacked, packed, (size_t)n_samples * (size_t)row_stride_bytes, 64)) return rc;
    HIPCHK(c, dcounts.alloc((size_t)n_windows * (size_t)n_samples * 3));
    if (int rc = census_on_device(c, dpacked.p, n_samples, row_stride_bytes, site_begin, site_end, n_windows, chunk, dcounts.p,
                                  nullptr))
      return rc;
    if (int rc = to_host(c, counts, dcounts)) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return ABN_OK;
  } catch (const std::bad_alloc&) {
    return set_err(c, ABN_ERR_HIP, "out of host memory");
  }
}
