// abn_sites_common*: the sites every sample shares, by genomic position (lifts the assumption of src/pedigree.rs:240, "the
// same sites are included in the datasets").  Kernels, the definition and the serial form: abn_sites_common.hpp.  The step
// runs in two halves around the one host read it needs: sites_common_match (runs, ends, match, scan, rank; then the order
// checks' verdict and n_common come to the host) and sites_common_gather (the aligned copies and the co-ordering check).
// The builders of abn_windows_create_aligned, abn_codes_create_aligned and abn_tiles_create reach both through sites_align
// (abn_resident.hip), between their merge and what their _parsed siblings do next.  The run tables (RunTables) are also
// the union step's (abn_sites_union.hip) and, over a handle's columns, abn_tiles.hip's.
#define ABN_SITES_COMMON_KERNELS  // (in front of abn_host.hpp, which includes abn_sites_common.hpp for CommonState)
#include "abn_host.hpp"

using namespace abn;

static int common_refuse(abn_ctx* c, const CommonRefusal& r) {
  if (!r.kind) return ABN_OK;
  return set_err(c, ABN_ERR_INVALID_ARG, "the samples cannot be aligned by position: " + common_refusal_text(r));
}

void RunTables::set(int n_samples, const int64_t* site_offset) {
  n = n_samples;
  site_off.assign(site_offset, site_offset + n + 1);
}

int RunTables::init(abn_ctx* c) {
  const size_t tables = (size_t)n * kCommonChroms;
  HIPCHK(c, dsite_off.alloc((size_t)n + 1));
  HIPCHK(c, run_begin.alloc(tables));
  HIPCHK(c, run_end.alloc(tables));
  HIPCHK(c, err.alloc(kCommonErrs));
  HIPCHK(c, hipMemcpyAsync(dsite_off.p, site_off.data(), dsite_off.bytes(), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemsetAsync(run_begin.p, 0x7f, run_begin.bytes(), c->stream));  // kCommonNone
  HIPCHK(c, hipMemsetAsync(run_end.p, 0, run_end.bytes(), c->stream));
  HIPCHK(c, hipMemsetAsync(err.p, 0x7f, err.bytes(), c->stream));
  return ABN_OK;
}

int RunTables::launch(abn_ctx* c, const CommonSites& in) {
  const long long S = sites();
  if (S <= 0) return ABN_OK;
  const dim3 grid((unsigned)((S + kCommonThreads - 1) / kCommonThreads)), threads(kCommonThreads);
  hipLaunchKernelGGL(abn_common_runs_kernel, grid, threads, 0, c->stream, in, (const long long*)dsite_off.p, n, run_begin.p,
                     err.p);
  HIPCHK(c, hipGetLastError());
  hipLaunchKernelGGL(abn_common_ends_kernel, grid, threads, 0, c->stream, in, (const long long*)dsite_off.p, n,
                     (const long long*)run_begin.p, run_end.p, err.p);
  HIPCHK(c, hipGetLastError());
  return ABN_OK;
}

int RunTables::refusal(abn_ctx* c, int first, int last, CommonRefusal* r) {
  long long host_err[kCommonErrs];
  HIPCHK(c, hipMemcpyAsync(host_err, err.p, sizeof host_err, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  *r = common_refusal(host_err, first, last, site_off.data(), n);
  return ABN_OK;
}

int abn::sites_common_scan(abn_ctx* c, uint32_t* data, uint32_t n) {
  hipLaunchKernelGGL(abn_common_scan_kernel, dim3(1), dim3(kCommonThreads), 0, c->stream, data, n);
  HIPCHK(c, hipGetLastError());
  return ABN_OK;
}

int abn::sites_common_match(abn_ctx* c, int n, const int64_t* site_offset, const CommonSites& in, uint8_t* dkeep,
                            CommonState& st) {
  RunTables& tab = st.tab;
  tab.set(n, site_offset);
  st.in = in;
  const long long S = tab.sites();
  st.probe = common_pick_probe(tab.site_off.data(), n);
  st.Lp = tab.site_off[(size_t)st.probe + 1] - tab.site_off[(size_t)st.probe];
  st.n_common = 0;
  if ((S + kCommonThreads - 1) / kCommonThreads > 0x7fffffffLL || st.Lp > 0xffffffffLL)
    return set_err(c, ABN_ERR_INVALID_ARG, "too many sites for one alignment");
  const size_t Lp = (size_t)st.Lp;
  const unsigned blocks = (unsigned)((Lp + kCommonThreads - 1) / kCommonThreads);
  if (!dkeep) {
    HIPCHK(c, st.keep_own.alloc((size_t)S));
    dkeep = st.keep_own.p;
  }
  st.keep = dkeep;
  HIPCHK(c, st.match.alloc((size_t)n * Lp));
  HIPCHK(c, st.src.alloc((size_t)n * Lp));
  HIPCHK(c, st.block.alloc((size_t)blocks + 1));
  if (int rc = st.ev.create(c)) return rc;
  if (int rc = tab.init(c)) return rc;
  if (S > 0) HIPCHK(c, hipMemsetAsync(dkeep, 0, (size_t)S, c->stream));
  HIPCHK(c, hipMemsetAsync(st.block.p, 0, st.block.bytes(), c->stream));  // (no probe site: the total is this 0)
  const dim3 threads(kCommonThreads);
  if (int rc = st.ev.record(c, 0)) return rc;
  if (int rc = tab.launch(c, in)) return rc;
  if (int rc = st.ev.record(c, 1)) return rc;
  uint8_t* probe_keep = dkeep + tab.site_off[(size_t)st.probe];
  if (Lp > 0) {
    hipLaunchKernelGGL(abn_common_match_kernel, dim3(blocks), threads, 0, c->stream, in, (const long long*)tab.dsite_off.p,
                       n, st.probe, st.Lp, (const long long*)tab.run_begin.p, (const long long*)tab.run_end.p, st.match.p,
                       probe_keep, st.block.p);
    HIPCHK(c, hipGetLastError());
  }
  if (int rc = st.ev.record(c, 2)) return rc;
  if (Lp > 0) {
    if (int rc = sites_common_scan(c, st.block.p, (uint32_t)blocks)) return rc;
    hipLaunchKernelGGL(abn_common_rank_kernel, dim3(blocks, (unsigned)n), threads, 0, c->stream,
                       (const uint8_t*)probe_keep, st.Lp, (const uint32_t*)st.block.p, (const uint32_t*)st.match.p, st.src.p);
    HIPCHK(c, hipGetLastError());
  }
  if (int rc = st.ev.record(c, 3)) return rc;
  uint32_t total = 0;
  CommonRefusal r;
  HIPCHK(c, hipMemcpyAsync(&total, st.block.p + blocks, 4, hipMemcpyDeviceToHost, c->stream));
  if (int rc = tab.refusal(c, kCommonSplitRun, kCommonBadKey, &r)) return rc;
  for (int k = 0; k < 3; ++k)
    if (int rc = st.ev.elapsed_ms(c, k, &st.ms[k])) return rc;
  if (int rc = common_refuse(c, r)) return rc;
  st.n_common = (long long)total;
  return ABN_OK;
}

int abn::sites_common_gather(abn_ctx* c, CommonState& st, const CommonGather& g) {
  if (int rc = st.ev.record(c, 4)) return rc;
  if (st.n_common > 0) {
    const dim3 grid((unsigned)((st.n_common + kCommonThreads - 1) / kCommonThreads), (unsigned)st.tab.n);
    hipLaunchKernelGGL(abn_common_gather_kernel, grid, dim3(kCommonThreads), 0, c->stream, st.in,
                       (const long long*)st.tab.dsite_off.p, st.probe, st.Lp, st.n_common, (const uint32_t*)st.src.p, st.keep,
                       g, st.tab.err.p);
    HIPCHK(c, hipGetLastError());
  }
  if (int rc = st.ev.record(c, 5)) return rc;
  CommonRefusal r;
  if (int rc = st.tab.refusal(c, kCommonNotCoordered, kCommonNotCoordered, &r)) return rc;
  if (int rc = st.ev.elapsed_ms(c, 4, &st.ms[3])) return rc;
  return common_refuse(c, r);
}

int abn::sites_keys_check(abn_ctx* c, int32_t n_samples, const int64_t* site_offset, const void* chromosome,
                          const void* start, const void* end, const void* strand, const void* out, const void* count) {
  if (!site_offset || !count || n_samples <= 0) return set_err(c, ABN_ERR_INVALID_ARG, "null/size");
  if (n_samples > 65535) return set_err(c, ABN_ERR_INVALID_ARG, "too many samples");
  if (int rc = site_offset_check(c, n_samples, site_offset)) return rc;
  if (site_offset[n_samples] > 0 && (!chromosome || !start || !end || !strand || !out))
    return set_err(c, ABN_ERR_INVALID_ARG, "null site arrays");
  return ABN_OK;
}

extern "C" int abn_sites_common_dev(abn_ctx* c, int32_t n_samples, const int64_t* site_offset, const void* dchromosome,
                                    const void* dstart, const void* dend, const void* dstrand, void* dkeep,
                                    int64_t* n_common) {
  if (!c) return ABN_ERR_INVALID_ARG;
  if (int rc = sites_keys_check(c, n_samples, site_offset, dchromosome, dstart, dend, dstrand, dkeep, n_common)) return rc;
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
  if (int rc = sites_keys_check(c, n_samples, site_offset, chromosome, start, end, strand, keep, n_common)) return rc;
  const size_t S = (size_t)site_offset[n_samples];
  HIPCHK(c, hipSetDevice(c->device));
  PoolScope pool_scope(c);
  SiteKeys key;
  DevBuf<uint8_t> dkeep;
  if (int rc = key.upload(c, S, chromosome, start, end, strand)) return rc;
  HIPCHK(c, dkeep.alloc(S));
  try {
    CommonState st;
    if (int rc = sites_common_match(c, n_samples, site_offset, key.keys(), dkeep.p, st)) return rc;
    if (int rc = sites_common_gather(c, st, CommonGather{})) return rc;
    if (S > 0) HIPCHK(c, hipMemcpyAsync(keep, dkeep.p, S, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    *n_common = st.n_common;
  } catch (const std::bad_alloc&) {
    return set_err(c, ABN_ERR_HIP, "out of host memory");
  }
  return ABN_OK;
}
