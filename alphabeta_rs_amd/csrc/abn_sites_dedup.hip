// abn_sites_dedup_keys*: the collapse of one sample's repeated keys on the device — flags, tile counts, their scan and the
// scatter of the kept records' indices — and what abn_sites_dedup (abn_sites.hip) launches around it: the gather of the
// kept records.  Kernels, policies and the serial forms: abn_sites_dedup.hpp; the flatten is the sort's
// (abn_sites_sort.hip), the scan is abn_parse_scan_kernel, launched by abn_sites.hip (sites_scan_rows).
#define ABN_SITES_DEDUP_KERNELS
#include "abn_host.hpp"

using namespace abn;

namespace {

unsigned dedup_grid(long long n) { return (unsigned)((n + kSortThreads - 1) / kSortThreads); }

// The flags and the compaction over n records read through `keys`; dorder has room for n entries and receives info4[1] of
// them.  info4 = {n, kept, repeated keys, disagreeing neighbours}; ms2 = the HIP-event ms of the flags (with BEST's walk)
// and of the compaction (count, scan, scatter).  A key outside its ranges and a descent, which the flags kernel finds, are
// refused before the compaction.  Returns after completion.
template <class Keys>
int dedup_run(abn_ctx* c, long long n, const Keys& keys, int policy, uint32_t* dorder, int64_t* info4, double* ms2) {
  info4[0] = n, info4[1] = info4[2] = info4[3] = 0;
  ms2[0] = ms2[1] = 0.0;
  if (n == 0) return ABN_OK;
  const long long tiles = sort_tiles(n);
  const unsigned blocks = std::min<unsigned>(kSortCheckBlocks, dedup_grid(n));
  DevBuf<uint8_t> dkeep;
  DevBuf<uint32_t> dpartial, dcount;
  EventPair ev;
  HIPCHK(c, dkeep.alloc((size_t)n));
  HIPCHK(c, dpartial.alloc((size_t)blocks * kDedupPartialWords));
  HIPCHK(c, dcount.alloc((size_t)tiles + 1));
  if (int rc = ev.begin(c, true)) return rc;
  hipLaunchKernelGGL(abn_dedup_flags_kernel<Keys>, dim3(blocks), dim3(kSortThreads), 0, c->stream, keys, n, policy, dkeep.p,
                     dpartial.p);
  HIPCHK(c, hipGetLastError());
  if (int rc = ev.end(c, &ms2[0])) return rc;
  std::vector<uint32_t> partial((size_t)blocks * kDedupPartialWords);
  if (int rc = to_host(c, partial.data(), dpartial)) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  DedupCheck check;
  for (unsigned g = 0; g < blocks; ++g) {
    const uint32_t* p = &partial[(size_t)g * kDedupPartialWords];
    DedupCheck one;
    one.descent = p[0], one.bad = p[1], one.repeated = p[2], one.disagreeing = p[3];
    check.add(one);
  }
  if (check.bad) return set_err(c, ABN_ERR_INVALID_ARG, "a chromosome outside 0..257 or a strand above 2");
  if (check.descent != kDedupNoDescent)
    return set_err(c, ABN_ERR_INVALID_ARG, "abn_sites_dedup: site " + std::to_string(check.descent) +
                                               " lies below its predecessor in canonical order: sort first (abn_sites_sort)");
  info4[2] = check.repeated, info4[3] = check.disagreeing;
  if (int rc = ev.begin(c, true)) return rc;
  hipLaunchKernelGGL(abn_dedup_count_kernel, dim3((unsigned)tiles), dim3(kSortThreads), 0, c->stream, (const uint8_t*)dkeep.p,
                     (uint32_t)n, dcount.p);
  HIPCHK(c, hipGetLastError());
  if (int rc = sites_scan_rows(c, dcount.p, 1u, (uint32_t)tiles, (uint32_t)tiles + 1u)) return rc;
  hipLaunchKernelGGL(abn_dedup_scatter_kernel, dim3((unsigned)tiles), dim3(kSortThreads), 0, c->stream, (const uint8_t*)dkeep.p,
                     (uint32_t)n, (const uint32_t*)dcount.p, (uint32_t)n, dorder);
  HIPCHK(c, hipGetLastError());
  if (int rc = ev.end(c, &ms2[1])) return rc;
  uint32_t kept = 0;
  if (int rc = to_host(c, &kept, dcount.p + tiles, sizeof kept)) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  info4[1] = kept;
  return ABN_OK;
}

int dedup_keys_args(abn_ctx* c, int64_t n, const void* chromosome, const void* start, const void* end, const void* strand,
                    const void* posteriormax, const void* status, int policy, const void* order, const void* info4) {
  if (n < 0 || !info4 || (n > 0 && (!chromosome || !start || !end || !strand || !posteriormax || !status || !order)))
    return set_err(c, ABN_ERR_INVALID_ARG, "null/size");
  if (!dedup_policy_valid(policy)) return set_err(c, ABN_ERR_INVALID_ARG, "abn_sites_dedup: a policy outside 0..3");
  if (n >= (int64_t)1 << 32) return set_err(c, ABN_ERR_INVALID_ARG, "abn_sites_dedup_keys: 2^32 keys or more");
  return ABN_OK;
}

}  // namespace

int abn::dedup_flat_dev(abn_ctx* c, long long n, const SortFlat& flat, int policy, uint32_t* dorder, int64_t* info4, double* ms2) {
  return dedup_run(c, n, DedupMeta{flat.meta, flat.start, flat.end, flat.posteriormax}, policy, dorder, info4, ms2);
}

int abn::dedup_gather_dev(abn_ctx* c, const SortFlat& in, const uint32_t* dorder, long long kept, long long n_in,
                          const ParseRecords& out) {
  if (kept == 0) return ABN_OK;
  hipLaunchKernelGGL(abn_dedup_gather_kernel, dim3(dedup_grid(kept)), dim3(kSortThreads), 0, c->stream, in, dorder, kept, n_in, out);
  HIPCHK(c, hipGetLastError());
  return ABN_OK;
}

extern "C" int abn_sites_dedup_keys_dev(abn_ctx* c, int64_t n, const void* dchromosome, const void* dstart, const void* dend,
                                        const void* dstrand, const void* dposteriormax, const void* dstatus, int policy,
                                        void* dorder, int64_t* info4, double* ms2) {
  if (!c) return ABN_ERR_INVALID_ARG;
  if (int rc = dedup_keys_args(c, n, dchromosome, dstart, dend, dstrand, dposteriormax, dstatus, policy, dorder, info4)) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  PoolScope pool_scope(c);
  double ms[2];
  try {
    if (int rc = dedup_run(c, n, DedupArrays{(const int32_t*)dchromosome, (const uint32_t*)dstart, (const uint32_t*)dend,
                                             (const uint8_t*)dstrand, (const double*)dposteriormax, (const uint8_t*)dstatus},
                           policy, (uint32_t*)dorder, info4, ms))
      return rc;
  } catch (const std::bad_alloc&) {
    return set_err(c, ABN_ERR_HIP, "out of host memory");
  }
  if (ms2) ms2[0] = ms[0], ms2[1] = ms[1];
  return ABN_OK;
}

extern "C" int abn_sites_dedup_keys(abn_ctx* c, int64_t n, const int32_t* chromosome, const uint32_t* start,
                                    const uint32_t* end, const uint8_t* strand, const double* posteriormax,
                                    const uint8_t* status, int policy, int64_t* order, int64_t* info4) {
  if (!c) return ABN_ERR_INVALID_ARG;
  if (int rc = dedup_keys_args(c, n, chromosome, start, end, strand, posteriormax, status, policy, order, info4)) return rc;
  for (int64_t i = 0; i < n; ++i)  // host-only, before any launch
    if (!sort_key_valid(chromosome[i], strand[i]))
      return set_err(c, ABN_ERR_INVALID_ARG, "a chromosome outside 0..257 or a strand above 2");
  if (n == 0) {
    info4[0] = info4[1] = info4[2] = info4[3] = 0;
    return ABN_OK;
  }
  HIPCHK(c, hipSetDevice(c->device));
  PoolScope pool_scope(c);
  try {
    const size_t N = (size_t)n;
    SiteKeys key;
    DevBuf<double> dpm;
    DevBuf<uint8_t> dstatus;
    DevBuf<uint32_t> dorder;
    double ms[2];
    if (int rc = key.upload(c, N, chromosome, start, end, strand)) return rc;
    if (int rc = upload(c, dpm, posteriormax, N)) return rc;
    if (int rc = upload(c, dstatus, status, N)) return rc;
    HIPCHK(c, dorder.alloc(N));
    if (int rc = dedup_run(c, n, DedupArrays{key.chrom.p, key.start.p, key.end.p, key.strand.p, dpm.p, dstatus.p}, policy,
                           dorder.p, info4, ms))
      return rc;
    const size_t kept = (size_t)info4[1];
    std::vector<uint32_t> o(kept);
    if (kept > 0) {
      if (int rc = to_host(c, o.data(), dorder.p, kept * sizeof(uint32_t))) return rc;
      HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    for (size_t k = 0; k < kept; ++k) order[k] = (int64_t)o[k];
  } catch (const std::bad_alloc&) {
    return set_err(c, ABN_ERR_HIP, "out of host memory");
  }
  return ABN_OK;
}
