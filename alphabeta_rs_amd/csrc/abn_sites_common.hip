// abn_sites_common*: the sites every sample shares, by genomic position (lifts the assumption of src/pedigree.rs:240, "the
// same sites are included in the datasets").  Kernels, the definition and the serial form: abn_sites_common.hpp.  The step
// runs in two halves around the one host read it needs: sites_common_match (runs, ends, match, scan, rank; then the order
// checks' verdict and n_common come to the host) and sites_common_gather (the aligned copies and the co-ordering check).
// abn_windows_create_aligned (abn_windows.hip) and abn_codes_create_aligned (abn_codes.hip) call both between their merge
// and what their _parsed siblings do next.
#define ABN_SITES_COMMON_KERNELS  // (in front of abn_host.hpp, which includes abn_sites_common.hpp for CommonState)
#include "abn_host.hpp"

using namespace abn;

CommonState::~CommonState() {
  for (hipEvent_t x : ev)
    if (x) (void)hipEventDestroy(x);
}

static int common_refuse(abn_ctx* c, const long long* err, int first, int last, const std::vector<long long>& site_off, int n) {
  const CommonRefusal r = common_refusal(err, first, last, site_off.data(), n);
  if (!r.kind) return ABN_OK;
  return set_err(c, ABN_ERR_INVALID_ARG, "the samples cannot be aligned by position: " + common_refusal_text(r));
}

int abn::sites_common_tables(abn_ctx* c, const CommonSites& in, const long long* dsite_off, int n, long long S,
                             long long* run_begin, long long* run_end, long long* err) {
  if (S <= 0) return ABN_OK;
  const dim3 grid((unsigned)((S + kCommonThreads - 1) / kCommonThreads)), threads(kCommonThreads);
  hipLaunchKernelGGL(abn_common_runs_kernel, grid, threads, 0, c->stream, in, dsite_off, n, run_begin, err);
  HIPCHK(c, hipGetLastError());
  hipLaunchKernelGGL(abn_common_ends_kernel, grid, threads, 0, c->stream, in, dsite_off, n, (const long long*)run_begin,
                     run_end, err);
  HIPCHK(c, hipGetLastError());
  return ABN_OK;
}

int abn::sites_common_scan(abn_ctx* c, uint32_t* data, uint32_t n) {
  hipLaunchKernelGGL(abn_common_scan_kernel, dim3(1), dim3(kCommonThreads), 0, c->stream, data, n);
  HIPCHK(c, hipGetLastError());
  return ABN_OK;
}

int abn::sites_common_match(abn_ctx* c, int n, const int64_t* site_offset, const CommonSites& in, uint8_t* dkeep,
                            CommonState& st) {
  st.n = n;
  st.in = in;
  st.site_off.assign(site_offset, site_offset + n + 1);
  const long long S = st.site_off[(size_t)n];
  st.probe = common_pick_probe(st.site_off.data(), n);
  st.Lp = st.site_off[(size_t)st.probe + 1] - st.site_off[(size_t)st.probe];
  st.n_common = 0;
  if ((S + kCommonThreads - 1) / kCommonThreads > 0x7fffffffLL || st.Lp > 0xffffffffLL)
    return set_err(c, ABN_ERR_INVALID_ARG, "too many sites for one alignment");
  const size_t Lp = (size_t)st.Lp, tables = (size_t)n * kCommonChroms;
  const unsigned blocks = (unsigned)((Lp + kCommonThreads - 1) / kCommonThreads);
  if (!dkeep) {
    HIPCHK(c, st.keep_own.alloc((size_t)S));
    dkeep = st.keep_own.p;
  }
  st.keep = dkeep;
  HIPCHK(c, st.dsite_off.alloc((size_t)n + 1));
  HIPCHK(c, st.run_begin.alloc(tables));
  HIPCHK(c, st.run_end.alloc(tables));
  HIPCHK(c, st.err.alloc(kCommonErrs));
  HIPCHK(c, st.match.alloc((size_t)n * Lp));
  HIPCHK(c, st.src.alloc((size_t)n * Lp));
  HIPCHK(c, st.block.alloc((size_t)blocks + 1));
  st.temp_bytes = st.keep_own.bytes() + st.dsite_off.bytes() + st.run_begin.bytes() + st.run_end.bytes() + st.err.bytes() +
                  st.match.bytes() + st.src.bytes() + st.block.bytes();
  for (int k = 0; k < 6; ++k)
    if (!st.ev[k]) HIPCHK(c, hipEventCreate(&st.ev[k]));
  HIPCHK(c, hipMemcpyAsync(st.dsite_off.p, st.site_off.data(), st.dsite_off.bytes(), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemsetAsync(st.run_begin.p, 0x7f, st.run_begin.bytes(), c->stream));  // kCommonNone
  HIPCHK(c, hipMemsetAsync(st.run_end.p, 0, st.run_end.bytes(), c->stream));
  HIPCHK(c, hipMemsetAsync(st.err.p, 0x7f, st.err.bytes(), c->stream));
  if (S > 0) HIPCHK(c, hipMemsetAsync(dkeep, 0, (size_t)S, c->stream));
  HIPCHK(c, hipMemsetAsync(st.block.p, 0, st.block.bytes(), c->stream));  // (no probe site: the total is this 0)
  const dim3 threads(kCommonThreads);
  HIPCHK(c, hipEventRecord(st.ev[0], c->stream));
  if (int rc = sites_common_tables(c, in, st.dsite_off.p, n, S, st.run_begin.p, st.run_end.p, st.err.p)) return rc;
  HIPCHK(c, hipEventRecord(st.ev[1], c->stream));
  uint8_t* probe_keep = dkeep + st.site_off[(size_t)st.probe];
  if (Lp > 0) {
    hipLaunchKernelGGL(abn_common_match_kernel, dim3(blocks), threads, 0, c->stream, in, (const long long*)st.dsite_off.p,
                       n, st.probe, st.Lp, (const long long*)st.run_begin.p, (const long long*)st.run_end.p, st.match.p,
                       probe_keep, st.block.p);
    HIPCHK(c, hipGetLastError());
  }
  HIPCHK(c, hipEventRecord(st.ev[2], c->stream));
  if (Lp > 0) {
    if (int rc = sites_common_scan(c, st.block.p, (uint32_t)blocks)) return rc;
    hipLaunchKernelGGL(abn_common_rank_kernel, dim3(blocks, (unsigned)n), threads, 0, c->stream,
                       (const uint8_t*)probe_keep, st.Lp, (const uint32_t*)st.block.p, (const uint32_t*)st.match.p, st.src.p);
    HIPCHK(c, hipGetLastError());
  }
  HIPCHK(c, hipEventRecord(st.ev[3], c->stream));
  long long err[kCommonErrs];
  uint32_t total = 0;
  HIPCHK(c, hipMemcpyAsync(err, st.err.p, sizeof err, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(&total, st.block.p + blocks, 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (int k = 0; k < 3; ++k) {
    float ms = 0.f;
    HIPCHK(c, hipEventElapsedTime(&ms, st.ev[k], st.ev[k + 1]));
    st.ms[k] = ms;
  }
  if (int rc = common_refuse(c, err, kCommonSplitRun, kCommonBadKey, st.site_off, n)) return rc;
  st.n_common = (long long)total;
  return ABN_OK;
}

int abn::sites_common_gather(abn_ctx* c, CommonState& st, const CommonGather& g) {
  HIPCHK(c, hipEventRecord(st.ev[4], c->stream));
  if (st.n_common > 0) {
    const dim3 grid((unsigned)((st.n_common + kCommonThreads - 1) / kCommonThreads), (unsigned)st.n);
    hipLaunchKernelGGL(abn_common_gather_kernel, grid, dim3(kCommonThreads), 0, c->stream, st.in,
                       (const long long*)st.dsite_off.p, st.probe, st.Lp, st.n_common, (const uint32_t*)st.src.p, st.keep, g,
                       st.err.p);
    HIPCHK(c, hipGetLastError());
  }
  HIPCHK(c, hipEventRecord(st.ev[5], c->stream));
  long long err[kCommonErrs];
  HIPCHK(c, hipMemcpyAsync(err, st.err.p, sizeof err, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  float ms = 0.f;
  HIPCHK(c, hipEventElapsedTime(&ms, st.ev[4], st.ev[5]));
  st.ms[3] = ms;
  return common_refuse(c, err, kCommonNotCoordered, kCommonNotCoordered, st.site_off, st.n);
}

static int common_check(abn_ctx* c, int32_t n_samples, const int64_t* site_offset, const void* chromosome, const void* start,
                        const void* end, const void* strand, const void* keep, const void* n_common) {
  if (!site_offset || !n_common || n_samples <= 0) return set_err(c, ABN_ERR_INVALID_ARG, "null/size");
  if (n_samples > 65535) return set_err(c, ABN_ERR_INVALID_ARG, "too many samples");
  if (site_offset[0] != 0) return set_err(c, ABN_ERR_INVALID_ARG, "site_offset[0] is not 0");
  for (int s = 0; s < n_samples; ++s)
    if (site_offset[s + 1] < site_offset[s] || site_offset[s + 1] - site_offset[s] > 0xffffffffLL)
      return set_err(c, ABN_ERR_INVALID_ARG, "site_offset is not ascending, or a sample of 2^32 sites or more");
  if (site_offset[n_samples] > 0 && (!chromosome || !start || !end || !strand || !keep))
    return set_err(c, ABN_ERR_INVALID_ARG, "null site arrays");
  return ABN_OK;
}

extern "C" int abn_sites_common_dev(abn_ctx* c, int32_t n_samples, const int64_t* site_offset, const void* dchromosome,
                                    const void* dstart, const void* dend, const void* dstrand, void* dkeep,
                                    int64_t* n_common) {
  if (!c) return ABN_ERR_INVALID_ARG;
  if (int rc = common_check(c, n_samples, site_offset, dchromosome, dstart, dend, dstrand, dkeep, n_common)) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  PoolScope pool_scope(c);
  try {
    CommonState st;
    if (int rc = sites_common_match(c, n_samples, site_offset, CommonSites{(const int32_t*)dchromosome, (const uint32_t*)dstart, (const uint32_t*)dend,
                                                        (const uint8_t*)dstrand},
                                    (uint8_t*)dkeep, st))
      return rc;
    if (int rc = sites_common_gather(c, st, CommonGather{})) return rc;
    *n_common = st.n_common;
  } catch (const std::bad_alloc&) {
    return set_err(c, ABN_ERR_HIP, "out of host memory");
  }
  return ABN_OK;
}

extern "C" int abn_sites_common(abn_ctx* c, int32_t n_samples, const int64_t* site_offset, const int32_t* chromosome,
                                const uint32_t* start, const uint32_t* end, const uint8_t* strand, uint8_t* keep,
                                int64_t* n_common) {
  if (!c) return ABN_ERR_INVALID_ARG;
  if (int rc = common_check(c, n_samples, site_offset, chromosome, start, end, strand, keep, n_common)) return rc;
  const size_t S = (size_t)site_offset[n_samples];
  HIPCHK(c, hipSetDevice(c->device));
  PoolScope pool_scope(c);
  DevBuf<int32_t> dchrom;
  DevBuf<uint32_t> dstart, dend;
  DevBuf<uint8_t> dstrand, dkeep;
  HIPCHK(c, dchrom.alloc(S));
  HIPCHK(c, dstart.alloc(S));
  HIPCHK(c, dend.alloc(S));
  HIPCHK(c, dstrand.alloc(S));
  HIPCHK(c, dkeep.alloc(S));
  if (S > 0) {
    HIPCHK(c, hipMemcpyAsync(dchrom.p, chromosome, S * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(dstart.p, start, S * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(dend.p, end, S * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(dstrand.p, strand, S, hipMemcpyHostToDevice, c->stream));
  }
  try {
    CommonState st;
    if (int rc = sites_common_match(c, n_samples, site_offset, CommonSites{dchrom.p, dstart.p, dend.p, dstrand.p}, dkeep.p, st))
      return rc;
    if (int rc = sites_common_gather(c, st, CommonGather{})) return rc;
    if (S > 0) HIPCHK(c, hipMemcpyAsync(keep, dkeep.p, S, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    *n_common = st.n_common;
  } catch (const std::bad_alloc&) {
    return set_err(c, ABN_ERR_HIP, "out of host memory");
  }
  return ABN_OK;
}
