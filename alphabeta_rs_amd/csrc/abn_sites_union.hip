// abn_sites_union*: the union of the samples' sites, by genomic position, with filtered placeholders where a sample lacks
// one (the per-pair comparison of src/pedigree.rs:240-254 on samples that hold different sites).  Kernels, the definition
// and the serial form: abn_sites_union.hpp.  The step runs in two halves around the caller's allocation, as the
// common-site step: sites_union_rank (runs, ends, owner, scan; the refusals, n_union and the run tables come to the host,
// which decides the chromosomes' order; base, rank, dest) and sites_union_gather (invert, gather).
// The builders of abn_windows_create_union, abn_codes_create_union and abn_tiles_create reach both through sites_align
// (abn_resident.hip), between their merge and what their _parsed siblings do next.  The run tables (RunTables: the runs /
// ends kernels) and the scan kernel are abn_sites_common.hip's.
#define ABN_SITES_UNION_KERNELS  // (in front of abn_host.hpp, which includes abn_sites_union.hpp for UnionState)
#include "abn_host.hpp"

using namespace abn;

static int union_refuse(abn_ctx* c, const CommonRefusal& r) {
  if (!r.kind) return ABN_OK;
  return set_err(c, ABN_ERR_INVALID_ARG, "the samples cannot be aligned by union: " + union_refusal_text(r));
}

int abn::sites_union_rank(abn_ctx* c, int n, const int64_t* site_offset, const CommonSites& in, uint32_t* ddest,
                          UnionState& st) {
  RunTables& tab = st.tab;
  tab.set(n, site_offset);
  st.in = in;
  st.n_union = 0;
  const long long S = tab.sites();
  if (S > 0xffffffffLL)  // (a site's index and n_union <= S fit a uint32_t)
    return set_err(c, ABN_ERR_INVALID_ARG, "too many sites for one alignment: the union holds at most 2^32 - 1");
  const unsigned blocks = (unsigned)((S + kCommonThreads - 1) / kCommonThreads);
  if (!ddest) {
    HIPCHK(c, st.dest_own.alloc((size_t)S));
    ddest = st.dest_own.p;
  }
  st.dest = ddest;
  HIPCHK(c, st.owner.alloc((size_t)S));
  HIPCHK(c, st.P.alloc((size_t)S + 1));
  HIPCHK(c, st.r.alloc((size_t)S));
  HIPCHK(c, st.block.alloc((size_t)blocks + 1));
  HIPCHK(c, st.order.alloc(kCommonChroms));
  HIPCHK(c, st.count.alloc(kCommonChroms));
  HIPCHK(c, st.base.alloc(kCommonChroms));
  if (int rc = st.ev.create(c)) return rc;
  if (int rc = tab.init(c)) return rc;
  HIPCHK(c, hipMemsetAsync(st.block.p, 0, st.block.bytes(), c->stream));  // (no site: n_union is this 0)
  HIPCHK(c, hipMemsetAsync(st.P.p, 0, 4, c->stream));                     // (no site: P[0] = P[S])
  HIPCHK(c, hipMemsetAsync(st.base.p, 0, st.base.bytes(), c->stream));
  const dim3 threads(kCommonThreads), grid(blocks);
  const long long* doff = tab.dsite_off.p;
  const long long *rb = tab.run_begin.p, *re = tab.run_end.p;
  if (int rc = st.ev.record(c, 0)) return rc;
  if (int rc = tab.launch(c, in)) return rc;
  if (int rc = st.ev.record(c, 1)) return rc;
  if (S > 0) {
    hipLaunchKernelGGL(abn_union_owner_kernel, grid, threads, 0, c->stream, in, doff, n, rb, re, st.owner.p, st.block.p);
    HIPCHK(c, hipGetLastError());
  }
  if (int rc = st.ev.record(c, 2)) return rc;
  if (S > 0) {
    if (int rc = sites_common_scan(c, st.block.p, (uint32_t)blocks)) return rc;
    hipLaunchKernelGGL(abn_union_prefix_kernel, grid, threads, 0, c->stream, S, (const uint32_t*)st.owner.p,
                       (const uint32_t*)st.block.p, (uint32_t)blocks, st.P.p);
    HIPCHK(c, hipGetLastError());
  }
  if (int rc = st.ev.record(c, 3)) return rc;
  uint32_t total = 0;
  std::vector<long long> run_begin(tab.run_begin.n);
  CommonRefusal refused;
  HIPCHK(c, hipMemcpyAsync(&total, st.block.p + blocks, 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(run_begin.data(), tab.run_begin.p, tab.run_begin.bytes(), hipMemcpyDeviceToHost, c->stream));
  if (int rc = tab.refusal(c, kCommonSplitRun, kCommonBadKey, &refused)) return rc;
  if (int rc = union_refuse(c, refused)) return rc;
  std::vector<int> order;
  if (int rc = union_refuse(c, union_order_refusal(run_begin.data(), tab.site_off.data(), n, order))) return rc;
  st.n_union = (long long)total;
  const uint32_t* P = st.P.p;
  if (int rc = st.ev.record(c, 4)) return rc;
  if (!order.empty()) {
    HIPCHK(c, hipMemcpyAsync(st.order.p, order.data(), order.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(abn_union_count_kernel, dim3((unsigned)order.size()), threads, 0, c->stream, P, rb, re, n,
                       (const int*)st.order.p, st.count.p);
    HIPCHK(c, hipGetLastError());
    hipLaunchKernelGGL(abn_union_base_kernel, dim3(1), dim3(64), 0, c->stream, (const uint32_t*)st.count.p,
                       (const int*)st.order.p, (int)order.size(), st.base.p);
    HIPCHK(c, hipGetLastError());
  }
  if (int rc = st.ev.record(c, 5)) return rc;
  if (S > 0) {
    hipLaunchKernelGGL(abn_union_rank_kernel, grid, threads, 0, c->stream, in, S, n, rb, re, (const uint32_t*)st.owner.p, P,
                       (const uint32_t*)st.base.p, st.r.p);
    HIPCHK(c, hipGetLastError());
  }
  if (int rc = st.ev.record(c, 6)) return rc;
  if (S > 0) {
    hipLaunchKernelGGL(abn_union_dest_kernel, grid, threads, 0, c->stream, S, (const uint32_t*)st.owner.p,
                       (const uint32_t*)st.r.p, ddest);
    HIPCHK(c, hipGetLastError());
  }
  if (int rc = st.ev.record(c, 7)) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));  // (`order` is read by the copy above until here)
  for (int k = 0; k < 3; ++k) {
    if (int rc = st.ev.elapsed_ms(c, k, &st.ms[k])) return rc;
    if (int rc = st.ev.elapsed_ms(c, k + 4, &st.ms[k + 3])) return rc;
  }
  return ABN_OK;
}

int abn::sites_union_gather(abn_ctx* c, UnionState& st, const CommonGather& g) {
  const long long S = st.tab.sites();
  HIPCHK(c, st.inv.alloc((size_t)st.tab.n * (size_t)st.n_union));
  HIPCHK(c, st.own_at.alloc((size_t)st.n_union));
  if (int rc = st.ev.record(c, 8)) return rc;
  if (st.n_union > 0) {
    HIPCHK(c, hipMemsetAsync(st.inv.p, 0xff, st.inv.bytes(), c->stream));  // kUnionNone
    hipLaunchKernelGGL(abn_union_invert_kernel, dim3((unsigned)((S + kCommonThreads - 1) / kCommonThreads)),
                       dim3(kCommonThreads), 0, c->stream, (const long long*)st.tab.dsite_off.p, st.tab.n, st.n_union,
                       (const uint32_t*)st.owner.p, (const uint32_t*)st.dest, st.inv.p, st.own_at.p);
    HIPCHK(c, hipGetLastError());
  }
  if (int rc = st.ev.record(c, 9)) return rc;
  if (st.n_union > 0) {
    const dim3 grid((unsigned)((st.n_union + kCommonThreads - 1) / kCommonThreads), (unsigned)st.tab.n);
    hipLaunchKernelGGL(abn_union_gather_kernel, grid, dim3(kCommonThreads), 0, c->stream, st.in,
                       (const long long*)st.tab.dsite_off.p, st.n_union, (const uint32_t*)st.inv.p,
                       (const uint32_t*)st.own_at.p, g);
    HIPCHK(c, hipGetLastError());
  }
  if (int rc = st.ev.record(c, 10)) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (int k = 0; k < 2; ++k)
    if (int rc = st.ev.elapsed_ms(c, k + 8, &st.ms[k + 6])) return rc;
  return ABN_OK;
}

extern "C" int abn_sites_union_dev(abn_ctx* c, int32_t n_samples, const int64_t* site_offset, const void* dchromosome,
                                   const void* dstart, const void* dend, const void* dstrand, void* ddest,
                                   int64_t* n_union) {
  if (!c) return ABN_ERR_INVALID_ARG;
  if (int rc = sites_keys_check(c, n_samples, site_offset, dchromosome, dstart, dend, dstrand, ddest, n_union)) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  PoolScope pool_scope(c);
  try {
    UnionState st;
    if (int rc = sites_union_rank(c, n_samples, site_offset,
                                  CommonSites{(const int32_t*)dchromosome, (const uint32_t*)dstart, (const uint32_t*)dend,
                                              (const uint8_t*)dstrand},
                                  (uint32_t*)ddest, st))
      return rc;
    *n_union = st.n_union;
  } catch (const std::bad_alloc&) {
    return set_err(c, ABN_ERR_HIP, "out of host memory");
  }
  return ABN_OK;
}

extern "C" int abn_sites_union(abn_ctx* c, int32_t n_samples, const int64_t* site_offset, const int32_t* chromosome,
                               const uint32_t* start, const uint32_t* end, const uint8_t* strand, uint32_t* dest,
                               int64_t* n_union) {
  if (!c) return ABN_ERR_INVALID_ARG;
  if (int rc = sites_keys_check(c, n_samples, site_offset, chromosome, start, end, strand, dest, n_union)) return rc;
  const size_t S = (size_t)site_offset[n_samples];
  HIPCHK(c, hipSetDevice(c->device));
  PoolScope pool_scope(c);
  SiteKeys key;
  DevBuf<uint32_t> ddest;
  if (int rc = key.upload(c, S, chromosome, start, end, strand)) return rc;
  HIPCHK(c, ddest.alloc(S));
  try {
    UnionState st;
    if (int rc = sites_union_rank(c, n_samples, site_offset, key.keys(), ddest.p, st)) return rc;
    if (S > 0) HIPCHK(c, hipMemcpyAsync(dest, ddest.p, S * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    *n_union = st.n_union;
  } catch (const std::bad_alloc&) {
    return set_err(c, ABN_ERR_HIP, "out of host memory");
  }
  return ABN_OK;
}
