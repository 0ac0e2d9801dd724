// Pedigree construction and the analysis of bootstrap tables, on the host and on the device:
// abn_pairwise_divergence*, abn_windows_*, abn_analyze, abn_analyze_batch*.
// The scan kernels are in abn_pairwise_mx.hpp, abn_pairwise_packed.hpp, abn_pairwise_windows.hpp and
// abn_pairwise_windows_packed.hpp, the window placement in abn_windows.hpp, the analysis kernel in abn_analyze.hpp; the
// fit path (abn_api.hip) does not include them.
#include "abn_host.hpp"
#include "abn_analyze.hpp"
#include "abn_pairwise_mx.hpp"
#include "abn_pairwise_packed.hpp"
#include "abn_pairwise_windows.hpp"
#include "abn_pairwise_windows_packed.hpp"
#include "abn_windows.hpp"

using namespace abn;

// ------------------------------------------------------------------------------------------------
// pedigree construction: pairwise divergence (src/pedigree.rs:210-261)
// ------------------------------------------------------------------------------------------------
// Exact integer Gram products on the matrix pipe (abn_pairwise_mx.hpp): any number of samples, the sample axis tiled in
// groups of 64; codes already on the device, outputs on the device (any may be null).
// the two HIP events around a call's kernels (kernel_ms), destroyed on every way out
struct EventPair {
  hipEvent_t e0 = nullptr, e1 = nullptr;
  EventPair() = default;
  EventPair(const EventPair&) = delete;
  EventPair& operator=(const EventPair&) = delete;
  ~EventPair() {
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
  }
};

constexpr long long kPmxMaxJobs = 8192;  // jobs per launch: 32 KiB of packed sums each (256 MiB of `partial`)

template <bool AL4>
static hipError_t launch_pairwise_mx(int nb, bool diag, unsigned grid, hipStream_t s, const PairMxArgs& a) {
  if (!diag) {
    hipLaunchKernelGGL((abn_pairwise_mx_kernel<4, false, AL4>), dim3(grid), dim3(kPmxThreads), 0, s, a);
  } else {
    switch (nb) {
      case 1: hipLaunchKernelGGL((abn_pairwise_mx_kernel<1, true, AL4>), dim3(grid), dim3(kPmxThreads), 0, s, a); break;
      case 2: hipLaunchKernelGGL((abn_pairwise_mx_kernel<2, true, AL4>), dim3(grid), dim3(kPmxThreads), 0, s, a); break;
      case 3: hipLaunchKernelGGL((abn_pairwise_mx_kernel<3, true, AL4>), dim3(grid), dim3(kPmxThreads), 0, s, a); break;
      default: hipLaunchKernelGGL((abn_pairwise_mx_kernel<4, true, AL4>), dim3(grid), dim3(kPmxThreads), 0, s, a); break;
    }
  }
  return hipGetLastError();
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
  if (kernel_ms) {
    HIPCHK(c, hipEventCreate(&ev.e0));
    HIPCHK(c, hipEventCreate(&ev.e1));
    HIPCHK(c, hipEventRecord(ev.e0, c->stream));
  }
  // workgroups per CU: two (eight wavefronts streaming per CU) once the scan is long enough to pay for twice the partial
  // rows; one below (byte codes, 50 x 2 M sites: 28.6 against 30.5 us; 50 x 32 M: 304 against 282 us)
  long long cu_diag = (long long)a.n * row_bytes >= (256ll << 20) ? 2 : 1, cu_off = 1;
#ifdef ABN_MEASUREMENT_KNOBS
  if (const char* e = getenv("ABN_PMX_CU_JOBS")) cu_diag = cu_off = std::max(1, atoi(e));
#endif
  const long long g = a.ngroups;
  int rc = pairwise_family(c, a, steps, L, true, g, cu_diag, pdiag, ddiff, dboth, ddval, launch);
  if (!rc) rc = pairwise_family(c, a, steps, L, false, g * (g - 1) / 2, cu_off, poff, ddiff, dboth, ddval, launch);
  if (rc) return rc;
  if (kernel_ms) {
    HIPCHK(c, hipEventRecord(ev.e1, c->stream));
    HIPCHK(c, hipEventSynchronize(ev.e1));
    float ms = 0.f;
    HIPCHK(c, hipEventElapsedTime(&ms, ev.e0, ev.e1));
    *kernel_ms = ms;
  }
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
  a.ngroups = (n + 63) / 64;
  const bool al4 = (L % 4 == 0) && ((uintptr_t)dcodes % 4 == 0);
  const int nb = a.ngroups == 1 ? (n + 15) / 16 : 4;
  return pairwise_scan_on_device(c, a, (L + 63) / 64, L, L, ddiff, dboth, ddval, kernel_ms,
                                 [&](bool diag, unsigned grid, const PairMxArgs& args) {
                                   return al4 ? launch_pairwise_mx<true>(nb, diag, grid, c->stream, args)
                                              : launch_pairwise_mx<false>(nb, diag, grid, c->stream, args);
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
  DevBuf<unsigned long long> ddiff, dboth;
  DevBuf<double> ddv;
  HIPCHK(c, dcodes.alloc(std::max<size_t>(n * (size_t)n_sites, 4)));
  HIPCHK(c, ddiff.alloc(npairs));
  HIPCHK(c, dboth.alloc(npairs));
  HIPCHK(c, ddv.alloc(npairs));
  if (n_sites > 0)
    HIPCHK(c, hipMemcpyAsync(dcodes.p, codes, n * (size_t)n_sites, hipMemcpyHostToDevice, c->stream));
  int rc = pairwise_mx_on_device(c, dcodes.p, n_samples, n_sites, ddiff.p, dboth.p, ddv.p, nullptr);
  if (rc) return rc;
  if (diff) HIPCHK(c, hipMemcpyAsync(diff, ddiff.p, ddiff.bytes(), hipMemcpyDeviceToHost, c->stream));
  if (both) HIPCHK(c, hipMemcpyAsync(both, dboth.p, dboth.bytes(), hipMemcpyDeviceToHost, c->stream));
  if (dvalue) HIPCHK(c, hipMemcpyAsync(dvalue, ddv.p, ddv.bytes(), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return ABN_OK;
}

// ------------------------------------------------------------------------------------------------
// the same on 2-bit packed codes (src/pedigree.rs:210-261; format: include/abneutral.h, abn_pack_codes)
// ------------------------------------------------------------------------------------------------
static hipError_t launch_pairwise_packed(int nb, bool diag, unsigned grid, hipStream_t s, const PairPackedArgs& a) {
  if (!diag) {
    hipLaunchKernelGGL((abn_pairwise_packed_kernel<4, false>), dim3(grid), dim3(kPmxThreads), 0, s, a);
  } else {
    switch (nb) {
      case 1: hipLaunchKernelGGL((abn_pairwise_packed_kernel<1, true>), dim3(grid), dim3(kPmxThreads), 0, s, a); break;
      case 2: hipLaunchKernelGGL((abn_pairwise_packed_kernel<2, true>), dim3(grid), dim3(kPmxThreads), 0, s, a); break;
      case 3: hipLaunchKernelGGL((abn_pairwise_packed_kernel<3, true>), dim3(grid), dim3(kPmxThreads), 0, s, a); break;
      default: hipLaunchKernelGGL((abn_pairwise_packed_kernel<4, true>), dim3(grid), dim3(kPmxThreads), 0, s, a); break;
    }
  }
  return hipGetLastError();
}

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
  a.ngroups = (n + 63) / 64;
  const int nb = a.ngroups == 1 ? (n + 15) / 16 : 4;
  // a chunk is a whole number of 64-byte super-steps of every row; the chunk rule is the byte scan's in those steps (a
  // wavefront's floor of four is then 16 matrix steps): the launch fills the GPU from a quarter of the bytes on
  return pairwise_scan_on_device(c, a, a.nk, L, 64 * a.nk, ddiff, dboth, ddval, kernel_ms,
                                 [&](bool diag, unsigned grid, const PairPackedArgs& args) {
                                   return launch_pairwise_packed(nb, diag, grid, c->stream, args);
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
  const size_t n = (size_t)n_samples, npairs = n * (n - 1) / 2, bytes = n * (size_t)row_stride_bytes;
  if (npairs == 0) return ABN_OK;
  HIPCHK(c, hipSetDevice(c->device));
  PoolScope pool_scope(c);
  DevBuf<uint8_t> dpacked;  // (device allocations are aligned far beyond the 16 bytes the kernel asks for)
  DevBuf<unsigned long long> ddiff, dboth;
  DevBuf<double> ddv;
  HIPCHK(c, dpacked.alloc(std::max<size_t>(bytes, 64)));
  HIPCHK(c, ddiff.alloc(npairs));
  HIPCHK(c, dboth.alloc(npairs));
  HIPCHK(c, ddv.alloc(npairs));
  if (bytes > 0) HIPCHK(c, hipMemcpyAsync(dpacked.p, packed, bytes, hipMemcpyHostToDevice, c->stream));
  int rc = pairwise_packed_on_device(c, dpacked.p, n_samples, n_sites, row_stride_bytes, ddiff.p, dboth.p, ddv.p, nullptr);
  if (rc) return rc;
  if (diff) HIPCHK(c, hipMemcpyAsync(diff, ddiff.p, ddiff.bytes(), hipMemcpyDeviceToHost, c->stream));
  if (both) HIPCHK(c, hipMemcpyAsync(both, dboth.p, dboth.bytes(), hipMemcpyDeviceToHost, c->stream));
  if (dvalue) HIPCHK(c, hipMemcpyAsync(dvalue, ddv.p, ddv.bytes(), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return ABN_OK;
}

// ------------------------------------------------------------------------------------------------
// the same for many windows of one code matrix (src/cli/metaprofile.rs:50-72 around src/pedigree.rs:210-261)
// ------------------------------------------------------------------------------------------------
template <bool AL4>
static hipError_t launch_pairwise_win(int nb, bool diag, unsigned grid, hipStream_t s, const PairWinArgs& a) {
  if (!diag) {
    hipLaunchKernelGGL((abn_pairwise_win_kernel<4, false, AL4>), dim3(grid), dim3(kPmxThreads), 0, s, a);
  } else {
    switch (nb) {
      case 1: hipLaunchKernelGGL((abn_pairwise_win_kernel<1, true, AL4>), dim3(grid), dim3(kPmxThreads), 0, s, a); break;
      case 2: hipLaunchKernelGGL((abn_pairwise_win_kernel<2, true, AL4>), dim3(grid), dim3(kPmxThreads), 0, s, a); break;
      case 3: hipLaunchKernelGGL((abn_pairwise_win_kernel<3, true, AL4>), dim3(grid), dim3(kPmxThreads), 0, s, a); break;
      default: hipLaunchKernelGGL((abn_pairwise_win_kernel<4, true, AL4>), dim3(grid), dim3(kPmxThreads), 0, s, a); break;
    }
  }
  return hipGetLastError();
}

// The jobs of one family of super-pairs over all windows, in launches ("slabs") of at most kPmxMaxJobs jobs; the chunks
// of one (window, super-pair) never straddle two slabs, so a slab's reduce launch finds all rows of its tasks.
// A window's chunks are cut at multiples of chunk[w] from its begin rounded down to `align` sites (1: byte codes, from the
// begin itself; 256: packed codes, whole super-steps); launch(diag, grid, args) starts the scan kernel of the format.
struct PairWinFamily {
  struct Slab { size_t job0, njobs, task0, ntasks, nrows; };
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
        if (cur.njobs + (size_t)nch > (size_t)kPmxMaxJobs) {
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
    HIPCHK(c, partial.alloc(max_rows * kPmxJobElems));
    if (!jobs.empty())
      HIPCHK(c, hipMemcpyAsync(djobs.p, jobs.data(), djobs.bytes(), hipMemcpyHostToDevice, c->stream));
    if (!tasks.empty())
      HIPCHK(c, hipMemcpyAsync(dtasks.p, tasks.data(), dtasks.bytes(), hipMemcpyHostToDevice, c->stream));
    return ABN_OK;
  }
  template <class Launch>
  int run(abn_ctx* c, PairWinArgs a, bool diag, Launch launch) {
    a.partial = partial.p;
    for (const Slab& s : slabs) {
      if (s.njobs == 0) continue;
      a.jobs = djobs.p + s.job0;
      HIPCHK(c, launch(diag, (unsigned)s.njobs, a));
      if (s.ntasks == 0) continue;
      hipLaunchKernelGGL(abn_pairwise_win_reduce_kernel, dim3((unsigned)(s.ntasks * 256)), dim3(16 * kPmxReduceGroups), 0,
                         c->stream, partial.p, dtasks.p + s.task0, a.n, a.ngroups, diag ? 1 : 0, a.diff, a.both,
                         a.dvalue);
      HIPCHK(c, hipGetLastError());
    }
    return ABN_OK;
  }
};

// Both families of a windows scan between the two events of kernel_ms: plan, upload the job tables, run.
template <class Launch>
static int pairwise_windows_run(abn_ctx* c, const PairWinArgs& a, const int64_t* begin, const int64_t* end, int W,
                                const std::vector<long long>& chunk, long long align, double* kernel_ms, Launch launch) {
  const long long g = a.ngroups;
  PairWinFamily fdiag, foff;  // (their host tables outlive the copies: the stream is synchronised below)
  fdiag.plan(g, begin, end, W, chunk, align);
  foff.plan(g * (g - 1) / 2, begin, end, W, chunk, align);
  int rc = fdiag.upload(c);
  if (!rc) rc = foff.upload(c);
  if (rc) return rc;
  EventPair ev;
  if (kernel_ms) {
    HIPCHK(c, hipEventCreate(&ev.e0));
    HIPCHK(c, hipEventCreate(&ev.e1));
    HIPCHK(c, hipEventRecord(ev.e0, c->stream));
  }
  rc = fdiag.run(c, a, true, launch);
  if (!rc) rc = foff.run(c, a, false, launch);
  if (rc) return rc;
  if (kernel_ms) {
    HIPCHK(c, hipEventRecord(ev.e1, c->stream));
    HIPCHK(c, hipEventSynchronize(ev.e1));
    float ms = 0.f;
    HIPCHK(c, hipEventElapsedTime(&ms, ev.e0, ev.e1));
    *kernel_ms = ms;
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));  // the job tables and the partial rows are freed on return
  return ABN_OK;
}

static int pairwise_windows_check(abn_ctx* c, const void* codes, int32_t n, int64_t row_stride, const int64_t* begin,
                                  const int64_t* end, int32_t W) {
  if (!codes || n <= 0 || row_stride < 0 || W < 0 || (W > 0 && (!begin || !end)))
    return set_err(c, ABN_ERR_INVALID_ARG, "null/size");
  if (n > 65535) return set_err(c, ABN_ERR_INVALID_ARG, "too many samples");
  for (int w = 0; w < W; ++w)
    if (begin[w] < 0 || begin[w] > end[w] || end[w] > row_stride)
      return set_err(c, ABN_ERR_INVALID_ARG, "window " + std::to_string(w) + " is not a column range of the rows");
  return ABN_OK;
}

static int pairwise_windows_on_device(abn_ctx* c, const uint8_t* dcodes, int n, long long row_stride,
                                      const int64_t* begin, const int64_t* end, int W, unsigned long long* ddiff,
                                      unsigned long long* dboth, double* ddval, double* kernel_ms) {
  PairWinArgs a{};
  a.codes = dcodes;
  a.row_stride = row_stride;
  a.n = n;
  a.ngroups = (n + 63) / 64;
  a.diff = ddiff;
  a.both = dboth;
  a.dvalue = ddval;
  bool al4 = (row_stride % 4 == 0) && ((uintptr_t)dcodes % 4 == 0);
  // sites per job of each window: kPmxWinChunkSites, more only where a window would otherwise need more rows of
  // `partial` than one launch keeps
  std::vector<long long> chunk((size_t)W);
  for (int w = 0; w < W; ++w) {
    al4 = al4 && begin[w] % 4 == 0;
    const long long L = end[w] - begin[w];
    long long ch = kPmxWinChunkSites;
    if ((L + ch - 1) / ch > kPmxMaxJobs) ch = ((L + kPmxMaxJobs - 1) / kPmxMaxJobs + 127) / 128 * 128;
    if (ch >= (1ll << 30)) return set_err(c, ABN_ERR_INVALID_ARG, "window too long");
    chunk[(size_t)w] = ch;
  }
  const int nb = a.ngroups == 1 ? (n + 15) / 16 : 4;
  return pairwise_windows_run(c, a, begin, end, W, chunk, 1, kernel_ms,
                              [&](bool diag, unsigned grid, const PairWinArgs& args) {
                                return al4 ? launch_pairwise_win<true>(nb, diag, grid, c->stream, args)
                                           : launch_pairwise_win<false>(nb, diag, grid, c->stream, args);
                              });
}

extern "C" int abn_pairwise_divergence_windows_dev(abn_ctx* c, const void* dev_codes, int32_t n_samples,
                                                   int64_t row_stride, const int64_t* site_begin,
                                                   const int64_t* site_end, int32_t n_windows, void* dev_diff,
                                                   void* dev_both, void* dev_dvalue, double* kernel_ms) {
  if (!c) return ABN_ERR_INVALID_ARG;
  if (int rc = pairwise_windows_check(c, dev_codes, n_samples, row_stride, site_begin, site_end, n_windows)) return rc;
  if (n_samples < 2 || n_windows == 0) return ABN_OK;
  HIPCHK(c, hipSetDevice(c->device));
  PoolScope pool_scope(c);
  return pairwise_windows_on_device(c, (const uint8_t*)dev_codes, n_samples, row_stride, site_begin, site_end, n_windows,
                                    (unsigned long long*)dev_diff, (unsigned long long*)dev_both, (double*)dev_dvalue,
                                    kernel_ms);
}

extern "C" int abn_pairwise_divergence_windows(abn_ctx* c, const uint8_t* codes, int32_t n_samples, int64_t row_stride,
                                               const int64_t* site_begin, const int64_t* site_end, int32_t n_windows,
                                               uint64_t* diff, uint64_t* both, double* dvalue) {
  if (!c) return ABN_ERR_INVALID_ARG;
  if (int rc = pairwise_windows_check(c, codes, n_samples, row_stride, site_begin, site_end, n_windows)) return rc;
  if (n_samples < 2 || n_windows == 0) return ABN_OK;
  const size_t n = (size_t)n_samples, nout = n * (n - 1) / 2 * (size_t)n_windows;
  HIPCHK(c, hipSetDevice(c->device));
  PoolScope pool_scope(c);
  DevBuf<uint8_t> dcodes;
  DevBuf<unsigned long long> ddiff, dboth;
  DevBuf<double> ddv;
  HIPCHK(c, dcodes.alloc(std::max<size_t>(n * (size_t)row_stride, 4)));
  if (diff) HIPCHK(c, ddiff.alloc(nout));
  if (both) HIPCHK(c, dboth.alloc(nout));
  if (dvalue) HIPCHK(c, ddv.alloc(nout));
  if (row_stride > 0)
    HIPCHK(c, hipMemcpyAsync(dcodes.p, codes, n * (size_t)row_stride, hipMemcpyHostToDevice, c->stream));
  int rc = pairwise_windows_on_device(c, dcodes.p, n_samples, row_stride, site_begin, site_end, n_windows, ddiff.p,
                                      dboth.p, ddv.p, nullptr);
  if (rc) return rc;
  if (diff) HIPCHK(c, hipMemcpyAsync(diff, ddiff.p, ddiff.bytes(), hipMemcpyDeviceToHost, c->stream));
  if (both) HIPCHK(c, hipMemcpyAsync(both, dboth.p, dboth.bytes(), hipMemcpyDeviceToHost, c->stream));
  if (dvalue) HIPCHK(c, hipMemcpyAsync(dvalue, ddv.p, ddv.bytes(), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return ABN_OK;
}

// ------------------------------------------------------------------------------------------------
// ... and for many windows of one 2-bit packed matrix (src/cli/metaprofile.rs:50-72 around src/pedigree.rs:210-261)
// ------------------------------------------------------------------------------------------------
static hipError_t launch_pairwise_win_packed(int nb, bool diag, unsigned grid, hipStream_t s, const PairWinArgs& a) {
  if (!diag) {
    hipLaunchKernelGGL((abn_pairwise_win_packed_kernel<4, false>), dim3(grid), dim3(kPmxThreads), 0, s, a);
  } else {
    switch (nb) {
      case 1: hipLaunchKernelGGL((abn_pairwise_win_packed_kernel<1, true>), dim3(grid), dim3(kPmxThreads), 0, s, a); break;
      case 2: hipLaunchKernelGGL((abn_pairwise_win_packed_kernel<2, true>), dim3(grid), dim3(kPmxThreads), 0, s, a); break;
      case 3: hipLaunchKernelGGL((abn_pairwise_win_packed_kernel<3, true>), dim3(grid), dim3(kPmxThreads), 0, s, a); break;
      default: hipLaunchKernelGGL((abn_pairwise_win_packed_kernel<4, true>), dim3(grid), dim3(kPmxThreads), 0, s, a); break;
    }
  }
  return hipGetLastError();
}

// Sites per job of each window: kPmxWinPackedChunkSites, more (whole super-steps) only where a window would otherwise
// need more rows of `partial` than one launch keeps.  Counted from the window's begin rounded down to a super-step.
static int pairwise_windows_packed_chunks(abn_ctx* c, const int64_t* begin, const int64_t* end, int W,
                                          std::vector<long long>& chunk) {
  chunk.resize((size_t)W);
  for (int w = 0; w < W; ++w) {
    const long long span = end[w] - (begin[w] - begin[w] % kPackedStepSites);
    long long ch = kPmxWinPackedChunkSites;
    if ((span + ch - 1) / ch > kPmxMaxJobs)
      ch = ((span + kPmxMaxJobs - 1) / kPmxMaxJobs + kPackedStepSites - 1) / kPackedStepSites * kPackedStepSites;
    if (ch >= (1ll << 30)) return set_err(c, ABN_ERR_INVALID_ARG, "window too long");
    chunk[(size_t)w] = ch;
  }
  return ABN_OK;
}

static int pairwise_windows_packed_check(abn_ctx* c, const void* packed, int32_t n, int64_t L, int64_t stride,
                                         const int64_t* begin, const int64_t* end, int32_t W,
                                         std::vector<long long>& chunk) {
  if (int rc = pairwise_packed_check(c, packed, n, L, stride)) return rc;
  if (W < 0 || (W > 0 && (!begin || !end))) return set_err(c, ABN_ERR_INVALID_ARG, "null/size");
  for (int w = 0; w < W; ++w)
    if (begin[w] < 0 || begin[w] > end[w] || end[w] > L)
      return set_err(c, ABN_ERR_INVALID_ARG, "window " + std::to_string(w) + " is not a column range of the rows");
  return pairwise_windows_packed_chunks(c, begin, end, W, chunk);
}

static int pairwise_windows_packed_on_device(abn_ctx* c, const uint8_t* dpacked, int n, long long stride,
                                             const int64_t* begin, const int64_t* end, int W,
                                             const std::vector<long long>& chunk, unsigned long long* ddiff,
                                             unsigned long long* dboth, double* ddval, double* kernel_ms) {
  PairWinArgs a{};
  a.codes = dpacked;
  a.row_stride = stride;
  a.n = n;
  a.ngroups = (n + 63) / 64;
  a.diff = ddiff;
  a.both = dboth;
  a.dvalue = ddval;
  const int nb = a.ngroups == 1 ? (n + 15) / 16 : 4;
  return pairwise_windows_run(c, a, begin, end, W, chunk, kPackedStepSites, kernel_ms,
                              [&](bool diag, unsigned grid, const PairWinArgs& args) {
                                return launch_pairwise_win_packed(nb, diag, grid, c->stream, args);
                              });
}

extern "C" int abn_pairwise_divergence_windows_packed_dev(abn_ctx* c, const void* dev_packed, int32_t n_samples,
                                                          int64_t n_sites, int64_t row_stride_bytes,
                                                          const int64_t* site_begin, const int64_t* site_end,
                                                          int32_t n_windows, void* dev_diff, void* dev_both,
                                                          void* dev_dvalue, double* kernel_ms) {
  if (!c) return ABN_ERR_INVALID_ARG;
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
  const size_t n = (size_t)n_samples, nout = n * (n - 1) / 2 * (size_t)n_windows, bytes = n * (size_t)row_stride_bytes;
  HIPCHK(c, hipSetDevice(c->device));
  PoolScope pool_scope(c);
  DevBuf<uint8_t> dpacked;  // (device allocations are aligned far beyond the 16 bytes the kernel asks for)
  DevBuf<unsigned long long> ddiff, dboth;
  DevBuf<double> ddv;
  HIPCHK(c, dpacked.alloc(std::max<size_t>(bytes, 64)));
  if (diff) HIPCHK(c, ddiff.alloc(nout));
  if (both) HIPCHK(c, dboth.alloc(nout));
  if (dvalue) HIPCHK(c, ddv.alloc(nout));
  if (bytes > 0) HIPCHK(c, hipMemcpyAsync(dpacked.p, packed, bytes, hipMemcpyHostToDevice, c->stream));
  int rc = pairwise_windows_packed_on_device(c, dpacked.p, n_samples, row_stride_bytes, site_begin, site_end, n_windows,
                                             chunk, ddiff.p, dboth.p, ddv.p, nullptr);
  if (rc) return rc;
  if (diff) HIPCHK(c, hipMemcpyAsync(diff, ddiff.p, ddiff.bytes(), hipMemcpyDeviceToHost, c->stream));
  if (both) HIPCHK(c, hipMemcpyAsync(both, dboth.p, dboth.bytes(), hipMemcpyDeviceToHost, c->stream));
  if (dvalue) HIPCHK(c, hipMemcpyAsync(dvalue, ddv.p, ddv.bytes(), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return ABN_OK;
}

// ------------------------------------------------------------------------------------------------
// window placement: methylome sites -> the packed matrix of the scan above (src/windows.rs:287-343 behind the gene choice,
// src/methylation_site.rs:423-490; kernels: abn_windows.hpp)
// ------------------------------------------------------------------------------------------------
struct abn_windows {
  abn_ctx* ctx = nullptr;
  int n = 0, W = 0;
  long long stride = 0;  // bytes per row of `packed`; the rows hold 4 * stride fields
  std::vector<int64_t> begin, end, count, kept;
  std::vector<int32_t> ragged;
  std::vector<double> level_sum, level_sum_kept;
  DevBuf<uint8_t> packed;  // [n x stride], device-resident between calls
};

static int windows_build(abn_windows* h, const abn_windows_params* p, const int64_t* site_offset, const uint32_t* pos,
                         const uint32_t* gene_start, const uint32_t* gene_end, const uint8_t* flags, const uint8_t* code,
                         const double* level) {
  abn_ctx* c = h->ctx;
  const int n = h->n, W = h->W;
  const size_t S = (size_t)site_offset[n], nW = (size_t)n * (size_t)W;
  WinParams P{};
  P.cutoff = (double)p->cutoff;
  P.step = (double)p->step;
  P.size = (double)p->size;
  P.absolute = p->absolute ? 1 : 0;
  P.n_region[0] = p->n_upstream;
  P.n_region[1] = p->n_gene;
  P.n_region[2] = p->n_downstream;
  P.first[0] = 0;
  P.first[1] = p->n_upstream;
  P.first[2] = p->n_upstream + p->n_gene;
  P.W = W;
  // the rank blocks: kWinBlockSites sites each, never across two samples
  std::vector<WinBlock> blocks;
  std::vector<int> block0((size_t)n + 1, 0);
  std::vector<long long> site0((size_t)n + 1);
  for (int s = 0; s <= n; ++s) site0[(size_t)s] = site_offset[s];
  for (int s = 0; s < n; ++s) {
    for (long long b = site_offset[s]; b < site_offset[s + 1]; b += kWinBlockSites)
      blocks.push_back(WinBlock{b, (int)std::min<long long>(kWinBlockSites, site_offset[s + 1] - b), s});
    block0[(size_t)s + 1] = (int)blocks.size();
  }
  const size_t NB = blocks.size();
  if ((double)NB * (double)std::max(W, 1) * 4.0 > 8e9)
    return set_err(c, ABN_ERR_INVALID_ARG, "too many sites x windows for one handle");

  DevBuf<uint32_t> dpos, dgs, dge, dhist, dlist;
  DevBuf<uint8_t> dflags, dcode;
  DevBuf<double> dlevel, dsum, dsumk;
  DevBuf<int2> dspan;
  DevBuf<WinBlock> dblocks;
  DevBuf<int> dblock0;
  DevBuf<long long> dsite0, dcount, dlistoff, dcol0, dkept;
  HIPCHK(c, dpos.alloc(S));
  HIPCHK(c, dgs.alloc(S));
  HIPCHK(c, dge.alloc(S));
  HIPCHK(c, dflags.alloc(S));
  HIPCHK(c, dcode.alloc(std::max<size_t>(S, 1)));
  HIPCHK(c, dlevel.alloc(std::max<size_t>(S, 1)));
  HIPCHK(c, dspan.alloc(S));
  HIPCHK(c, dblocks.alloc(NB));
  HIPCHK(c, dblock0.alloc((size_t)n + 1));
  HIPCHK(c, dsite0.alloc((size_t)n + 1));
  HIPCHK(c, dhist.alloc(std::max<size_t>(NB * (size_t)W, 1)));
  HIPCHK(c, dcount.alloc(std::max<size_t>(nW, 1)));
  if (S > 0) {
    HIPCHK(c, hipMemcpyAsync(dpos.p, pos, S * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(dgs.p, gene_start, S * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(dge.p, gene_end, S * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(dflags.p, flags, S, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(dcode.p, code, S, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(dlevel.p, level, S * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(dblocks.p, blocks.data(), dblocks.bytes(), hipMemcpyHostToDevice, c->stream));
  }
  HIPCHK(c, hipMemcpyAsync(dblock0.p, block0.data(), dblock0.bytes(), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(dsite0.p, site0.data(), dsite0.bytes(), hipMemcpyHostToDevice, c->stream));
  auto grid_of = [](size_t items) { return dim3((unsigned)((items + kWinThreads - 1) / kWinThreads)); };
  if (S > 0 && W > 0) {
    hipLaunchKernelGGL(abn_windows_place_kernel, grid_of(S), dim3(kWinThreads), 0, c->stream, dpos.p, dgs.p, dge.p,
                       dflags.p, (long long)S, P, dspan.p);
    HIPCHK(c, hipGetLastError());
    hipLaunchKernelGGL(abn_windows_rank_kernel<0>, dim3((unsigned)NB), dim3(kWinThreads), 0, c->stream, dspan.p,
                       dblocks.p, (int)NB, W, dhist.p, (const long long*)nullptr, dsite0.p, (uint32_t*)nullptr);
    HIPCHK(c, hipGetLastError());
  }
  h->count.assign(nW, 0);
  if (nW > 0) {
    hipLaunchKernelGGL(abn_windows_scan_kernel, grid_of(nW), dim3(kWinThreads), 0, c->stream, dhist.p, dblock0.p,
                       (int)NB, n, W, dcount.p);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(h->count.data(), dcount.p, nW * 8, hipMemcpyDeviceToHost, c->stream));
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));

  // the layout of layout_packed_call (host/pedigree_build.hpp): a window's columns begin at a multiple of 256 sites and
  // take ceil(sites / 256) * 64 bytes of every row; a ragged window takes none; at least one super-step per row
  std::vector<long long> list_off(nW + 1, 0), col0((size_t)W + 1, 0);
  for (size_t i = 0; i < nW; ++i) list_off[i + 1] = list_off[i] + h->count[i];
  h->begin.assign((size_t)W, 0);
  h->end.assign((size_t)W, 0);
  h->ragged.assign((size_t)W, 0);
  long long off = 0;  // bytes into the row
  for (int w = 0; w < W; ++w) {
    const long long L0 = h->count[(size_t)w];
    for (int s = 1; s < n; ++s)
      if (h->count[(size_t)s * W + w] != L0) h->ragged[(size_t)w] = 1;
    const long long L = h->ragged[(size_t)w] ? 0 : L0;
    col0[(size_t)w] = off / 4;
    h->begin[(size_t)w] = 4 * off;
    h->end[(size_t)w] = 4 * off + L;
    off += (L + 255) / 256 * 64;
  }
  col0[(size_t)W] = off / 4;
  h->stride = std::max<long long>(off, 64);
  const size_t row_dwords = (size_t)h->stride / 4, total = (size_t)list_off[nW];
  if (((size_t)n * row_dwords + kWinThreads - 1) / kWinThreads > 0x7fffffffull)
    return set_err(c, ABN_ERR_INVALID_ARG, "packed matrix too large for one handle");

  HIPCHK(c, dlistoff.alloc(nW + 1));
  HIPCHK(c, dcol0.alloc((size_t)W + 1));
  HIPCHK(c, dlist.alloc(std::max<size_t>(total, 1)));
  HIPCHK(c, dsum.alloc(std::max<size_t>(nW, 1)));
  HIPCHK(c, dsumk.alloc(std::max<size_t>(nW, 1)));
  HIPCHK(c, dkept.alloc(std::max<size_t>(nW, 1)));
  HIPCHK(c, h->packed.alloc((size_t)n * (size_t)h->stride));
  HIPCHK(c, hipMemcpyAsync(dlistoff.p, list_off.data(), dlistoff.bytes(), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(dcol0.p, col0.data(), dcol0.bytes(), hipMemcpyHostToDevice, c->stream));
  if (S > 0 && W > 0) {
    hipLaunchKernelGGL(abn_windows_rank_kernel<1>, dim3((unsigned)NB), dim3(kWinThreads), 0, c->stream, dspan.p,
                       dblocks.p, (int)NB, W, dhist.p, dlistoff.p, dsite0.p, dlist.p);
    HIPCHK(c, hipGetLastError());
  }
  hipLaunchKernelGGL(abn_windows_pack_kernel, grid_of((size_t)n * row_dwords), dim3(kWinThreads), 0, c->stream, dcode.p,
                     dlist.p, dlistoff.p, dcount.p, dsite0.p, dcol0.p, W, n, (long long)row_dwords,
                     (uint32_t*)h->packed.p);
  HIPCHK(c, hipGetLastError());
  h->level_sum.assign(nW, 0.0);
  h->level_sum_kept.assign(nW, 0.0);
  h->kept.assign(nW, 0);
  if (nW > 0) {
    hipLaunchKernelGGL(abn_windows_sums_kernel, grid_of(nW), dim3(kWinThreads), 0, c->stream, dcode.p, dlevel.p, dlist.p,
                       dlistoff.p, dcount.p, dsite0.p, W, n, dsum.p, dsumk.p, dkept.p);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(h->level_sum.data(), dsum.p, nW * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(h->level_sum_kept.data(), dsumk.p, nW * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(h->kept.data(), dkept.p, nW * 8, hipMemcpyDeviceToHost, c->stream));
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));  // the staging buffers are freed on return
  return ABN_OK;
}

extern "C" int abn_windows_create(abn_ctx* c, const abn_windows_params* p, int32_t n_samples, const int64_t* site_offset,
                                  const uint32_t* pos, const uint32_t* gene_start, const uint32_t* gene_end,
                                  const uint8_t* flags, const uint8_t* code, const double* level, abn_windows** out) {
  if (!c) return ABN_ERR_INVALID_ARG;
  if (out) *out = nullptr;
  if (!p || !out || !site_offset || n_samples <= 0) return set_err(c, ABN_ERR_INVALID_ARG, "null/size");
  if (n_samples > 65535) return set_err(c, ABN_ERR_INVALID_ARG, "too many samples");
  if (p->step == 0) return set_err(c, ABN_ERR_INVALID_ARG, "window step 0");
  if (p->n_upstream < 0 || p->n_gene < 0 || p->n_downstream < 0 ||
      (long long)p->n_upstream + p->n_gene + p->n_downstream > (1 << 20))
    return set_err(c, ABN_ERR_INVALID_ARG, "window counts");
  if (site_offset[0] != 0) return set_err(c, ABN_ERR_INVALID_ARG, "site_offset[0] is not 0");
  for (int s = 0; s < n_samples; ++s)
    if (site_offset[s + 1] < site_offset[s] || site_offset[s + 1] - site_offset[s] > 0xffffffffLL)
      return set_err(c, ABN_ERR_INVALID_ARG, "site_offset is not ascending, or a sample of 2^32 sites or more");
  if (site_offset[n_samples] > 0 && (!pos || !gene_start || !gene_end || !flags || !code || !level))
    return set_err(c, ABN_ERR_INVALID_ARG, "null site arrays");
  HIPCHK(c, hipSetDevice(c->device));
  PoolScope pool_scope(c);
  std::unique_ptr<abn_windows> h(new (std::nothrow) abn_windows);
  if (!h) return set_err(c, ABN_ERR_HIP, "out of host memory");
  h->ctx = c;
  h->n = n_samples;
  h->W = p->n_upstream + p->n_gene + p->n_downstream;
  try {
    if (int rc = windows_build(h.get(), p, site_offset, pos, gene_start, gene_end, flags, code, level)) return rc;
  } catch (const std::bad_alloc&) {
    return set_err(c, ABN_ERR_HIP, "out of host memory");
  }
  *out = h.release();
  return ABN_OK;
}

extern "C" int abn_windows_destroy(abn_windows* h) {
  if (!h) return ABN_ERR_INVALID_ARG;
  (void)hipSetDevice(h->ctx->device);
  delete h;
  return ABN_OK;
}

extern "C" int abn_windows_info(const abn_windows* h, int32_t* n_windows, int64_t* row_stride, int64_t* n_sites) {
  if (!h) return ABN_ERR_INVALID_ARG;
  if (n_windows) *n_windows = h->W;
  if (row_stride) *row_stride = h->stride;
  if (n_sites) *n_sites = 4 * h->stride;
  return ABN_OK;
}

extern "C" int abn_windows_stats(const abn_windows* h, int64_t* count, double* level_sum, double* level_sum_kept,
                                 int64_t* kept) {
  if (!h) return ABN_ERR_INVALID_ARG;
  if (count) std::copy(h->count.begin(), h->count.end(), count);
  if (level_sum) std::copy(h->level_sum.begin(), h->level_sum.end(), level_sum);
  if (level_sum_kept) std::copy(h->level_sum_kept.begin(), h->level_sum_kept.end(), level_sum_kept);
  if (kept) std::copy(h->kept.begin(), h->kept.end(), kept);
  return ABN_OK;
}

extern "C" int abn_windows_layout(const abn_windows* h, int64_t* begin, int64_t* end, int32_t* ragged) {
  if (!h) return ABN_ERR_INVALID_ARG;
  if (begin) std::copy(h->begin.begin(), h->begin.end(), begin);
  if (end) std::copy(h->end.begin(), h->end.end(), end);
  if (ragged) std::copy(h->ragged.begin(), h->ragged.end(), ragged);
  return ABN_OK;
}

extern "C" int abn_windows_packed_device_ptr(abn_windows* h, void** dev_ptr) {
  if (!h || !dev_ptr) return ABN_ERR_INVALID_ARG;
  *dev_ptr = h->packed.p;
  return ABN_OK;
}

extern "C" int abn_windows_packed(abn_windows* h, uint8_t* host_out) {
  if (!h) return ABN_ERR_INVALID_ARG;
  abn_ctx* c = h->ctx;
  if (!host_out) return set_err(c, ABN_ERR_INVALID_ARG, "null/size");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipMemcpyAsync(host_out, h->packed.p, h->packed.bytes(), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return ABN_OK;
}

extern "C" int abn_windows_pairwise(abn_windows* h, uint64_t* diff, uint64_t* both, double* dvalue) {
  if (!h) return ABN_ERR_INVALID_ARG;
  abn_ctx* c = h->ctx;
  const size_t n = (size_t)h->n, nout = n * (n - 1) / 2 * (size_t)h->W;
  if (nout == 0) return ABN_OK;
  std::vector<long long> chunk;
  if (int rc = pairwise_windows_packed_check(c, h->packed.p, h->n, 4 * h->stride, h->stride, h->begin.data(),
                                             h->end.data(), h->W, chunk))
    return rc;
  HIPCHK(c, hipSetDevice(c->device));
  PoolScope pool_scope(c);
  DevBuf<unsigned long long> ddiff, dboth;
  DevBuf<double> ddv;
  if (diff) HIPCHK(c, ddiff.alloc(nout));
  if (both) HIPCHK(c, dboth.alloc(nout));
  if (dvalue) HIPCHK(c, ddv.alloc(nout));
  if (int rc = pairwise_windows_packed_on_device(c, h->packed.p, h->n, h->stride, h->begin.data(), h->end.data(), h->W,
                                                 chunk, ddiff.p, dboth.p, ddv.p, nullptr))
    return rc;
  if (diff) HIPCHK(c, hipMemcpyAsync(diff, ddiff.p, ddiff.bytes(), hipMemcpyDeviceToHost, c->stream));
  if (both) HIPCHK(c, hipMemcpyAsync(both, dboth.p, dboth.bytes(), hipMemcpyDeviceToHost, c->stream));
  if (dvalue) HIPCHK(c, hipMemcpyAsync(dvalue, ddv.p, ddv.bytes(), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return ABN_OK;
}

// ------------------------------------------------------------------------------------------------
// src/analysis.rs:50-98 on the host (ndarray mean / Welford std with mul_add, ndarray-stats Linear CI)
// ------------------------------------------------------------------------------------------------
extern "C" int abn_analyze(const double* raw, int64_t n_boot, double* out32) {
  if (!raw || !out32 || n_boot <= 0) return ABN_ERR_INVALID_ARG;
  const size_t B = (size_t)n_boot;
  // the quantiles sort with `<`: a table with a NaN entry or a NaN beta / alpha is refused, out32 untouched (the
  // reference converts to n64, which rejects NaN, :57-58)
  for (size_t i = 0; i < B; ++i)
    if (abn_analyze_row_is_bad(raw + 7 * i)) return ABN_ERR_NO_FINITE_FIT;
  std::vector<double> col(B), sorted(B);
  static const int src_col[8] = {0, 1, -1, 2, 3, 4, 5, 6};
  for (int k = 0; k < 8; ++k) {
    const int cidx = src_col[k];
    for (size_t i = 0; i < B; ++i)
      col[i] = cidx < 0 ? raw[7 * i + 1] / raw[7 * i + 0] : raw[7 * i + (size_t)cidx];  // beta / alpha, :54
    double mean;
    if (cidx < 0) {  // contiguous Array1 -> ndarray's eight-lane unrolled fold
      double part[8] = {0, 0, 0, 0, 0, 0, 0, 0};
      size_t i = 0;
      for (; i + 8 <= B; i += 8)
        for (int q = 0; q < 8; ++q) part[q] = part[q] + col[i + (size_t)q];
      double acc = 0.0;
      acc = acc + (part[0] + part[4]);
      acc = acc + (part[1] + part[5]);
      acc = acc + (part[2] + part[6]);
      acc = acc + (part[3] + part[7]);
      for (; i < B; ++i) acc = acc + col[i];
      mean = acc / (double)B;
    } else {  // strided column view -> plain fold
      double acc = 0.0;
      for (size_t i = 0; i < B; ++i) acc = acc + col[i];
      mean = acc / (double)B;
    }
    double wmean = 0.0, sum_sq = 0.0;
    for (size_t i = 0; i < B; ++i) {
      const double delta = col[i] - wmean;
      wmean = wmean + delta / (double)(i + 1);
      sum_sq = std::fma(col[i] - wmean, delta, sum_sq);
    }
    const double sd = std::sqrt(sum_sq / ((double)B - 1.0));
    sorted = col;
    std::sort(sorted.begin(), sorted.end());
    const double qs[2] = {0.025, 0.975};
    double ci[2];
    for (int q = 0; q < 2; ++q) {
      const double fi = qs[q] * (double)(B - 1);
      const size_t lo = (size_t)std::floor(fi), hi = (size_t)std::ceil(fi);
      const double frac = fi - std::trunc(fi);
      ci[q] = sorted[lo] + frac * (sorted[hi] - sorted[lo]);
    }
    out32[k] = mean;
    out32[8 + k] = sd;
    out32[16 + k] = ci[0];
    out32[24 + k] = ci[1];
  }
  return ABN_OK;
}

// ------------------------------------------------------------------------------------------------
// src/analysis.rs:50-98 on the device, every window of a table in one launch (abn_analyze.hpp)
// ------------------------------------------------------------------------------------------------
static int analyze_check(abn_ctx* c, const void* raw, int32_t W, int64_t B, const void* out) {
  if (!raw || !out || W < 0 || B <= 0) return set_err(c, ABN_ERR_INVALID_ARG, "null/size");
  if (B > 0x7fffffffLL) return set_err(c, ABN_ERR_INVALID_ARG, "n_boot above 2^31 - 1");
  return ABN_OK;
}

static int analyze_enqueue(abn_ctx* c, const double* draw, int W, long long B, double* dout, int32_t* dfb) {
  for (int w0 = 0; w0 < W; w0 += kAnMaxWindowsPerLaunch) {
    const int wn = std::min(kAnMaxWindowsPerLaunch, W - w0);
    hipLaunchKernelGGL(abn_analyze_kernel, dim3((unsigned)wn * 8u), dim3(kAnThreads), 0, c->stream,
                       AnalyzeArgs{draw, dout, dfb, B, w0});
    HIPCHK(c, hipGetLastError());
  }
  return ABN_OK;
}

// ABN_ERR_NO_FINITE_FIT once everything has been written, as abn_plan_download
static int analyze_verdict(abn_ctx* c, const int32_t* fb, int W) {
  for (int w = 0; w < W; ++w)
    if (fb[w] >= 0)
      return set_err(c, ABN_ERR_NO_FINITE_FIT, "window " + std::to_string(w) + ": bootstrap " + std::to_string(fb[w]) +
                                                   " has no finite fit: its analysis is NaN");
  return ABN_OK;
}

int abn::analyze_device_table(abn_ctx* c, const double* draw, int32_t W, int64_t B, double* out, int32_t* first_bad) {
  if (int rc = analyze_check(c, draw, W, B, out)) return rc;
  if (W == 0) return ABN_OK;
  HIPCHK(c, hipSetDevice(c->device));
  PoolScope pool_scope(c);
  DevBuf<double> dout;
  DevBuf<int32_t> dfb;
  HIPCHK(c, dout.alloc((size_t)W * 32));
  HIPCHK(c, dfb.alloc((size_t)W));
  if (int rc = analyze_enqueue(c, draw, W, B, dout.p, dfb.p)) return rc;
  std::vector<int32_t> fb((size_t)W);
  HIPCHK(c, hipMemcpyAsync(out, dout.p, dout.bytes(), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(fb.data(), dfb.p, dfb.bytes(), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (first_bad) std::copy(fb.begin(), fb.end(), first_bad);
  return analyze_verdict(c, fb.data(), W);
}

extern "C" int abn_analyze_batch_dev(abn_ctx* c, const void* dev_raw, int32_t n_windows, int64_t n_boot, void* dev_out,
                                     void* dev_first_bad, double* kernel_ms) {
  if (!c) return ABN_ERR_INVALID_ARG;
  if (int rc = analyze_check(c, dev_raw, n_windows, n_boot, dev_out)) return rc;
  if (n_windows == 0) return ABN_OK;
  HIPCHK(c, hipSetDevice(c->device));
  PoolScope pool_scope(c);
  DevBuf<int32_t> dfb;  // the verdict needs first_bad whether or not the caller wants it
  if (!dev_first_bad) HIPCHK(c, dfb.alloc((size_t)n_windows));
  int32_t* fbp = dev_first_bad ? (int32_t*)dev_first_bad : dfb.p;
  EventPair ev;
  if (kernel_ms) {
    HIPCHK(c, hipEventCreate(&ev.e0));
    HIPCHK(c, hipEventCreate(&ev.e1));
    HIPCHK(c, hipEventRecord(ev.e0, c->stream));
  }
  if (int rc = analyze_enqueue(c, (const double*)dev_raw, n_windows, n_boot, (double*)dev_out, fbp)) return rc;
  if (kernel_ms) HIPCHK(c, hipEventRecord(ev.e1, c->stream));
  std::vector<int32_t> fb((size_t)n_windows);
  HIPCHK(c, hipMemcpyAsync(fb.data(), fbp, fb.size() * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (kernel_ms) {
    float ms = 0.f;
    HIPCHK(c, hipEventElapsedTime(&ms, ev.e0, ev.e1));
    *kernel_ms = ms;
  }
  return analyze_verdict(c, fb.data(), n_windows);
}

extern "C" int abn_analyze_batch(abn_ctx* c, const double* raw, int32_t n_windows, int64_t n_boot, double* out,
                                 int32_t* first_bad) {
  if (!c) return ABN_ERR_INVALID_ARG;
  if (int rc = analyze_check(c, raw, n_windows, n_boot, out)) return rc;
  if (n_windows == 0) return ABN_OK;
  HIPCHK(c, hipSetDevice(c->device));
  PoolScope pool_scope(c);
  DevBuf<double> draw;
  HIPCHK(c, draw.alloc((size_t)n_windows * (size_t)n_boot * 7));
  HIPCHK(c, hipMemcpyAsync(draw.p, raw, draw.bytes(), hipMemcpyHostToDevice, c->stream));
  return analyze_device_table(c, draw.p, n_windows, n_boot, out, first_bad);  // synchronises: draw is freed after it
}
