// abn_codes_*: the pedigree build's code matrix and rc_meth_lvl folds from resident parse results (src/pedigree.rs:138-178
// behind from_methylome_file_line, and the status bytes DMatrix::from reads, :210-261).  Kernels and arithmetic:
// abn_codes.hpp; the merge launches are abn_sites.hip's (the records are its handle's), the scan abn_pairwise.hip's, the
// common-site step of abn_codes_create_aligned abn_sites_common.hip's, the union step of abn_codes_create_union
// abn_sites_union.hip's; the handles' refusals, the merge loops and the alignment's dispatch are abn_resident.hip's, shared
// with abn_windows.hip and abn_tiles.hip, and so are the handle's shell (handle_create, handle_destroy, handle_packed) and
// the upload of the pack's offsets (PackOffsets), abn_host.hpp's.
#include "abn_host.hpp"
#define ABN_CODES_KERNELS
#include "abn_codes.hpp"

using namespace abn;

struct abn_codes {
  abn_ctx* ctx = nullptr;
  int n = 0;
  long long stride = 0;     // bytes per row of `packed`
  int64_t max_sites = 0;    // of the longest sample
  bool same_len = true;
  std::vector<int64_t> count, kept;  // [n]
  std::vector<double> level_sum_kept;
  double ms[4] = {0.0, 0.0, 0.0, 0.0};  // merge records, merge inserted, pack, fold
  AlignReport report;                   // abn_codes_common, abn_codes_union
  DevBuf<uint8_t> packed;               // [n x stride], device-resident between calls
};

// the pack kernel over n rows of row_dwords dwords (for abn_tiles.hip too): on the context's stream, nothing waited for
int abn::codes_pack_dev(abn_ctx* c, const uint8_t* dcode, const long long* dcode_off, const long long* dsite_off, int n,
                        long long row_dwords, uint8_t* dpacked) {
  const unsigned grid = (unsigned)(((long long)n * row_dwords + kCodesThreads - 1) / kCodesThreads);
  hipLaunchKernelGGL(abn_codes_pack_kernel, dim3(grid), dim3(kCodesThreads), 0, c->stream, dcode, dcode_off, dsite_off, n,
                     row_dwords, (uint32_t*)dpacked);
  HIPCHK(c, hipGetLastError());
  return ABN_OK;
}

// merge, pack, fold; the merged arrays (9 bytes per site) live only in here.  With `align` the merge is the full one, keys
// included (and the reduced one behind it, for the merged bytes: merge_code has no kCodeCounted), and the sites every
// sample shares (abn_sites_common.hpp; kAlignPosition) or the union of the samples' sites with filtered placeholders
// (abn_sites_union.hpp; kAlignUnion) are gathered out of it into the arrays the pack and the fold read.
static int codes_build(abn_codes* h, double filter, abn_sites* const* samples, int align) {
  abn_ctx* c = h->ctx;
  const int n = h->n;
  const int64_t* before = h->report.before.data();
  // the prologue and the alignment: the keyed merge, untimed (ms has no slot for it), and the match or the ranks
  MergedSites m;
  Alignment a;
  if (align) {
    if (int rc = m.alloc(c, n, before)) return rc;
    if (int rc = m.merge_keyed(c, samples, filter, nullptr)) return rc;
    if (int rc = sites_align(c, align, n, m.off.data(), m.keys(), a)) return rc;
    h->count.assign((size_t)n, a.each);  // from here on the handle is one of n samples of n_common (n_union) sites
    h->max_sites = a.each;
    h->same_len = true;
  }
  PackOffsets off;  // the samples may differ in length: the fold reads the offsets too
  std::vector<int64_t>& site_off = off.site;
  std::vector<int64_t>& code_off = off.code;
  site_off.assign((size_t)n + 1, 0), code_off.assign((size_t)n + 1, 0);
  for (int s = 0; s < n; ++s) {
    site_off[(size_t)s + 1] = site_off[(size_t)s] + h->count[(size_t)s];
    code_off[(size_t)s + 1] = code_off[(size_t)s] + (h->count[(size_t)s] + 15) / 16 * 16;  // whole 16-byte loads of the pack
  }
  h->stride = std::max<long long>(abn_packed_row_stride(h->max_sites), 64);  // no site: still one super-step per row
  const long long row_dwords = h->stride / 4;
  if (((long long)n * row_dwords + kCodesThreads - 1) / kCodesThreads > 0x7fffffffLL)
    return set_err(c, ABN_ERR_INVALID_ARG, "packed matrix too large for one handle");

  DevBuf<uint8_t> dcode;
  DevBuf<double> dlevel, dsum;
  DevBuf<long long> dkept;
  HIPCHK(c, dcode.alloc(std::max<size_t>((size_t)code_off[(size_t)n], 16)));
  HIPCHK(c, dlevel.alloc(std::max<size_t>((size_t)site_off[(size_t)n], 1)));
  HIPCHK(c, dsum.alloc((size_t)n));
  HIPCHK(c, dkept.alloc((size_t)n));
  HIPCHK(c, h->packed.alloc((size_t)n * (size_t)h->stride));
  if (int rc = off.upload(c)) return rc;

  // the reduced merge, timed as ms[0..1]: into the merged arrays under an alignment, else straight into what the pack and
  // the fold read
  Events<5> ev;
  if (int rc = ev.create(c)) return rc;
  const CodeTargets packed_from{dcode.p, code_off.data(), dlevel.p, site_off.data()};
  if (int rc = m.merge_codes(c, n, samples, before, filter, align ? nullptr : &packed_from, ev.e)) return rc;
  if (align) {  // the gather (returns after completion; the events below still bracket the pack and the fold)
    const CommonGather g{m.code.p, m.level.p, nullptr, nullptr, nullptr, nullptr, dlevel.p, dcode.p, code_off[1]};
    if (int rc = sites_align_gather(c, a, g)) return rc;
    sites_align_report(a, h->report);
  }
  // the builder's own: pack and fold
  if (int rc = ev.record(c, 2)) return rc;
  if (int rc = codes_pack_dev(c, dcode.p, off.dcode.p, off.dsite.p, n, row_dwords, h->packed.p)) return rc;
  if (int rc = ev.record(c, 3)) return rc;
  hipLaunchKernelGGL(abn_codes_fold_kernel, dim3((unsigned)n), dim3(kCodesWave), 0, c->stream, dcode.p, dlevel.p,
                     off.dcode.p, off.dsite.p, dsum.p, dkept.p);
  HIPCHK(c, hipGetLastError());
  if (int rc = ev.record(c, 4)) return rc;
  std::vector<long long> kept((size_t)n);
  h->level_sum_kept.assign((size_t)n, 0.0);
  HIPCHK(c, hipMemcpyAsync(h->level_sum_kept.data(), dsum.p, dsum.bytes(), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(kept.data(), dkept.p, dkept.bytes(), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));  // the merged arrays are freed on return
  h->kept.assign(kept.begin(), kept.end());
  for (int k = 0; k < 4; ++k)
    if (int rc = ev.elapsed_ms(c, k, &h->ms[k])) return rc;
  return ABN_OK;
}

static int codes_create_parsed(abn_ctx* c, double posterior_max_filter, int32_t n_samples, abn_sites* const* samples,
                               int align, abn_codes** out) {
  if (!c) return ABN_ERR_INVALID_ARG;
  if (out) *out = nullptr;
  if (!out || !samples || n_samples <= 0) return set_err(c, ABN_ERR_INVALID_ARG, "null/size");
  if (n_samples > 65535) return set_err(c, ABN_ERR_INVALID_ARG, "too many samples");
  return handle_create(c, n_samples, out, [&](abn_codes* h) {
    h->count.assign((size_t)n_samples, 0);
    if (int rc = resident_counts(c, n_samples, samples, h->count.data())) return rc;
    for (int64_t count : h->count) {
      h->max_sites = std::max(h->max_sites, count);
      if (count != h->count[0]) h->same_len = false;
    }
    h->report.before = h->count;
    return codes_build(h, posterior_max_filter, samples, align);
  });
}

extern "C" int abn_codes_create_parsed(abn_ctx* c, double posterior_max_filter, int32_t n_samples,
                                       abn_sites* const* samples, abn_codes** out) {
  return codes_create_parsed(c, posterior_max_filter, n_samples, samples, kAlignNone, out);
}

extern "C" int abn_codes_create_aligned(abn_ctx* c, double posterior_max_filter, int32_t n_samples,
                                        abn_sites* const* samples, abn_codes** out) {
  return codes_create_parsed(c, posterior_max_filter, n_samples, samples, kAlignPosition, out);
}

extern "C" int abn_codes_create_union(abn_ctx* c, double posterior_max_filter, int32_t n_samples,
                                      abn_sites* const* samples, abn_codes** out) {
  return codes_create_parsed(c, posterior_max_filter, n_samples, samples, kAlignUnion, out);
}

extern "C" int abn_codes_common(const abn_codes* h, int64_t* before, int64_t* n_common, double* ms4) {
  return h ? h->report.common(before, n_common, ms4) : ABN_ERR_INVALID_ARG;
}

extern "C" int abn_codes_union(const abn_codes* h, int64_t* before, int64_t* n_union, double* ms8) {
  return h ? h->report.unite(before, n_union, ms8) : ABN_ERR_INVALID_ARG;
}

extern "C" int abn_codes_destroy(abn_codes* h) { return handle_destroy(h); }

extern "C" int abn_codes_info(const abn_codes* h, int32_t* n_samples, int64_t* n_sites, int64_t* row_stride_bytes,
                              int32_t* same_len) {
  if (!h) return ABN_ERR_INVALID_ARG;
  if (n_samples) *n_samples = h->n;
  if (n_sites) *n_sites = h->max_sites;
  if (row_stride_bytes) *row_stride_bytes = h->stride;
  if (same_len) *same_len = h->same_len ? 1 : 0;
  return ABN_OK;
}

extern "C" int abn_codes_stats(const abn_codes* h, int64_t* count, double* level_sum_kept, int64_t* kept) {
  if (!h) return ABN_ERR_INVALID_ARG;
  if (count) std::copy(h->count.begin(), h->count.end(), count);
  if (level_sum_kept) std::copy(h->level_sum_kept.begin(), h->level_sum_kept.end(), level_sum_kept);
  if (kept) std::copy(h->kept.begin(), h->kept.end(), kept);
  return ABN_OK;
}

extern "C" int abn_codes_packed(abn_codes* h, uint8_t* host_out) { return handle_packed(h, host_out); }

extern "C" int abn_codes_packed_device_ptr(abn_codes* h, void** dev_ptr) {
  if (!h || !dev_ptr) return ABN_ERR_INVALID_ARG;
  *dev_ptr = h->packed.p;
  return ABN_OK;
}

extern "C" int abn_codes_pairwise(abn_codes* h, uint64_t* diff, uint64_t* both, double* dvalue) {
  if (!h) return ABN_ERR_INVALID_ARG;
  abn_ctx* c = h->ctx;
  if (!h->same_len)
    return set_err(c, ABN_ERR_INVALID_ARG, "the samples differ in length: the pairwise scan needs the same number of sites in each");
  const size_t n = (size_t)h->n, npairs = n * (n - 1) / 2;
  if (npairs == 0) return ABN_OK;
  HIPCHK(c, hipSetDevice(c->device));
  PoolScope pool_scope(c);
  return pairwise_to_host(c, npairs, diff, both, dvalue, [&](auto* dd, auto* db, auto* dv) {
    return abn_pairwise_divergence_packed_dev(c, h->packed.p, h->n, h->max_sites, h->stride, dd, db, dv, nullptr);
  });
}

extern "C" int abn_codes_transitions(abn_codes* h, uint64_t* table) {
  if (!h) return ABN_ERR_INVALID_ARG;
  abn_ctx* c = h->ctx;
  if (!h->same_len)
    return set_err(c, ABN_ERR_INVALID_ARG, "the samples differ in length: the pairwise scan needs the same number of sites in each");
  if (h->n < 2) return ABN_OK;
  HIPCHK(c, hipSetDevice(c->device));
  PoolScope pool_scope(c);
  const int64_t begin = 0, end = h->max_sites;  // the whole matrix is one window
  return transitions_windows_packed_to_host(c, h->packed.p, h->n, h->max_sites, h->stride, &begin, &end, 1, table);
}

extern "C" int abn_codes_kernel_ms(const abn_codes* h, double* ms4) {
  if (!h || !ms4) return ABN_ERR_INVALID_ARG;
  std::copy(h->ms, h->ms + 4, ms4);
  return ABN_OK;
}
