// The front end the consumers of resident methylomes share — abn_windows_create_parsed / _aligned / _union
// (abn_windows.hip), abn_codes_create_parsed / _aligned / _union (abn_codes.hip) and abn_tiles_create (abn_tiles.hip): the
// refusals of their abn_sites handles, the merge of every sample's records on the device (its launches are
// abn_sites.hip's), and the optional alignment of the merged arrays — the common-site step (abn_sites_common.hip) or the
// union step (abn_sites_union.hip) — with its gather and its report.  Host code only: no kernel is defined here.  What
// they share behind the front end — the handle's shell and the upload of a pack's offsets — is inline in abn_host.hpp.
#include "abn_host.hpp"

using namespace abn;

int abn::resident_counts(abn_ctx* c, int32_t n_samples, abn_sites* const* samples, int64_t* counts) {
  for (int s = 0; s < n_samples; ++s) {
    if (!samples[s]) return set_err(c, ABN_ERR_INVALID_ARG, "a null sites handle");
    if (!sites_ctx(samples[s])) return set_err(c, ABN_ERR_INVALID_ARG, "a sites handle in the host form (abn_sites_parse)");
    if (sites_ctx(samples[s]) != c) return set_err(c, ABN_ERR_INVALID_ARG, "a sites handle of another context");
    counts[s] = sites_merged_count(samples[s]);
    if (counts[s] < 0)
      return set_err(c, ABN_ERR_INVALID_ARG, "a sites handle with deferred lines and no abn_sites_insert");
  }
  return ABN_OK;
}

int SiteKeys::alloc(abn_ctx* c, size_t S) {
  HIPCHK(c, chrom.alloc(S));
  HIPCHK(c, start.alloc(S));
  HIPCHK(c, end.alloc(S));
  HIPCHK(c, strand.alloc(S));
  return ABN_OK;
}

int SiteKeys::upload(abn_ctx* c, size_t S, const int32_t* chromosome, const uint32_t* start_, const uint32_t* end_,
                     const uint8_t* strand_) {
  if (int rc = alloc(c, S)) return rc;
  if (S == 0) return ABN_OK;
  HIPCHK(c, hipMemcpyAsync(chrom.p, chromosome, S * 4, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(start.p, start_, S * 4, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(end.p, end_, S * 4, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(strand.p, strand_, S, hipMemcpyHostToDevice, c->stream));
  return ABN_OK;
}

int MergedSites::alloc(abn_ctx* c, int n_keyed, const int64_t* count) {
  off.assign((size_t)n_keyed + 1, 0);
  for (int s = 0; s < n_keyed; ++s) off[(size_t)s + 1] = off[(size_t)s] + count[s];
  const size_t S = std::max<size_t>((size_t)off[(size_t)n_keyed], 1);
  if (int rc = SiteKeys::alloc(c, S)) return rc;
  HIPCHK(c, code.alloc(S));
  HIPCHK(c, level.alloc(S));
  return ABN_OK;
}

int MergedSites::merge_keyed(abn_ctx* c, abn_sites* const* samples, double filter, const hipEvent_t* marks) {
  const int n_keyed = (int)off.size() - 1;
  for (int pass = 0; pass < 2; ++pass) {  // the fields kernels of every sample, then the insert kernels
    if (marks) HIPCHK(c, hipEventRecord(marks[pass], c->stream));
    for (int s = 0; s < n_keyed; ++s) {
      const size_t o = (size_t)off[(size_t)s];
      if (off[(size_t)s + 1] == off[(size_t)s]) continue;
      if (int rc = sites_merge_dev(samples[s], pass == 1, filter, chrom.p + o, start.p + o, end.p + o, strand.p + o,
                                   code.p + o, level.p + o))
        return rc;
    }
  }
  if (marks) HIPCHK(c, hipEventRecord(marks[2], c->stream));
  return ABN_OK;
}

int MergedSites::merge_codes(abn_ctx* c, int n, abn_sites* const* samples, const int64_t* before, double filter,
                             const CodeTargets* to, const hipEvent_t* marks) {
  const CodeTargets own{code.p, off.data(), level.p, off.data()};
  if (!to) to = &own;
  for (int pass = 0; pass < 2; ++pass) {  // the fields kernels of every sample, then the insert kernels
    if (marks) HIPCHK(c, hipEventRecord(marks[pass], c->stream));
    for (int s = 0; s < n; ++s) {
      if (before[s] == 0) continue;
      if (int rc = sites_merge_codes_dev(samples[s], pass == 1, filter, to->code + to->code_off[s], to->level + to->level_off[s]))
        return rc;
    }
  }
  return ABN_OK;
}

int abn::sites_align(abn_ctx* c, int mode, int n, const int64_t* site_offset, const CommonSites& keys, Alignment& a) {
  a.mode = mode;
  if (mode == kAlignUnion) {
    if (int rc = sites_union_rank(c, n, site_offset, keys, nullptr, a.unite)) return rc;
    a.each = a.unite.n_union;
  } else {
    if (int rc = sites_common_match(c, n, site_offset, keys, nullptr, a.common)) return rc;
    a.each = a.common.n_common;
  }
  return ABN_OK;
}

int abn::sites_align_gather(abn_ctx* c, Alignment& a, const CommonGather& g) {
  return a.mode == kAlignUnion ? sites_union_gather(c, a.unite, g) : sites_common_gather(c, a.common, g);
}

void abn::sites_align_report(const Alignment& a, AlignReport& r) {
  if (a.mode == kAlignUnion) {
    r.n_union = a.each;
    std::copy(a.unite.ms, a.unite.ms + kUnionPasses, r.union_ms);
  } else {
    r.n_common = a.each;
    std::copy(a.common.ms, a.common.ms + 4, r.common_ms);
  }
}
