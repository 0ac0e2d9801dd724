// abn_windows_*: the window-placement handle.  Kernels: abn_windows.hpp; the scan of the placed windows
// (abn_windows_pairwise) is abn_pairwise.hip's, the gene choice of abn_windows_create_sites abn_genes.hip's; what stands in
// front of the gene choice of abn_windows_create_parsed / _aligned / _union — the resident handles' refusals, the merge of
// their parse results (abn_sites.hip's launches), and between that merge and the gene choice the common-site step
// (abn_sites_common.hip) or the union step (abn_sites_union.hip) — is abn_resident.hip's, shared with abn_codes.hip and
// abn_tiles.hip; so is the handle's shell (handle_create, handle_destroy, handle_packed), abn_host.hpp's.
#include "abn_host.hpp"
#include "abn_windows.hpp"

using namespace abn;

// ------------------------------------------------------------------------------------------------
// window placement: methylome sites -> the packed matrix of the windows scan (src/windows.rs:287-343 behind the gene choice,
// src/methylation_site.rs:423-490; kernels: abn_windows.hpp)
// ------------------------------------------------------------------------------------------------
struct abn_windows {
  abn_ctx* ctx = nullptr;
  int n = 0, W = 0;
  long long stride = 0;  // bytes per row of `packed`; the rows hold 4 * stride fields
  std::vector<int64_t> begin, end, count, kept;
  std::vector<int32_t> ragged;
  std::vector<double> level_sum, level_sum_kept;
  double merge_ms[2] = {0.0, 0.0};  // abn_windows_create_parsed: its fields and insert kernels
  AlignReport report;               // abn_windows_common, abn_windows_union
  DevBuf<uint8_t> packed;  // [n x stride], device-resident between calls
};

// The handle from DEVICE site arrays ([site_offset[n]] each; none is read when there are no sites): place, rank, pack, sum
static int windows_build_dev(abn_windows* h, const abn_windows_params* p, const int64_t* site_offset, const uint32_t* dpos,
                             const uint32_t* dgs, const uint32_t* dge, const uint8_t* dflags, const uint8_t* dcode,
                             const double* dlevel) {
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

  DevBuf<uint32_t> dhist, dlist;
  DevBuf<double> dsum, dsumk;
  DevBuf<int2> dspan;
  DevBuf<WinBlock> dblocks;
  DevBuf<int> dblock0;
  DevBuf<long long> dsite0, dcount, dlistoff, dcol0, dkept;
  HIPCHK(c, dspan.alloc(S));
  HIPCHK(c, dblocks.alloc(NB));
  HIPCHK(c, dblock0.alloc((size_t)n + 1));
  HIPCHK(c, dsite0.alloc((size_t)n + 1));
  HIPCHK(c, dhist.alloc(std::max<size_t>(NB * (size_t)W, 1)));
  HIPCHK(c, dcount.alloc(std::max<size_t>(nW, 1)));
  if (S > 0) HIPCHK(c, hipMemcpyAsync(dblocks.p, blocks.data(), dblocks.bytes(), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(dblock0.p, block0.data(), dblock0.bytes(), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(dsite0.p, site0.data(), dsite0.bytes(), hipMemcpyHostToDevice, c->stream));
  auto grid_of = [](size_t items) { return dim3((unsigned)((items + kWinThreads - 1) / kWinThreads)); };
  if (S > 0 && W > 0) {
    hipLaunchKernelGGL(abn_windows_place_kernel, grid_of(S), dim3(kWinThreads), 0, c->stream, dpos, dgs, dge,
                       dflags, (long long)S, P, dspan.p);
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
  hipLaunchKernelGGL(abn_windows_pack_kernel, grid_of((size_t)n * row_dwords), dim3(kWinThreads), 0, c->stream, dcode,
                     dlist.p, dlistoff.p, dcount.p, dsite0.p, dcol0.p, W, n, (long long)row_dwords,
                     (uint32_t*)h->packed.p);
  HIPCHK(c, hipGetLastError());
  h->level_sum.assign(nW, 0.0);
  h->level_sum_kept.assign(nW, 0.0);
  h->kept.assign(nW, 0);
  if (nW > 0) {
    hipLaunchKernelGGL(abn_windows_sums_kernel, grid_of(nW), dim3(kWinThreads), 0, c->stream, dcode, dlevel, dlist.p,
                       dlistoff.p, dcount.p, dsite0.p, W, n, dsum.p, dsumk.p, dkept.p);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(h->level_sum.data(), dsum.p, nW * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(h->level_sum_kept.data(), dsumk.p, nW * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(h->kept.data(), dkept.p, nW * 8, hipMemcpyDeviceToHost, c->stream));
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));  // the staging buffers are freed on return
  return ABN_OK;
}

// ... from HOST site arrays: the upload in front of windows_build_dev
static int windows_build(abn_windows* h, const abn_windows_params* p, const int64_t* site_offset, const uint32_t* pos,
                         const uint32_t* gene_start, const uint32_t* gene_end, const uint8_t* flags, const uint8_t* code,
                         const double* level) {
  abn_ctx* c = h->ctx;
  const size_t S = (size_t)site_offset[h->n];
  DevBuf<uint32_t> dpos, dgs, dge;
  DevBuf<uint8_t> dflags, dcode;
  DevBuf<double> dlevel;
  HIPCHK(c, dpos.alloc(S));
  HIPCHK(c, dgs.alloc(S));
  HIPCHK(c, dge.alloc(S));
  HIPCHK(c, dflags.alloc(S));
  HIPCHK(c, dcode.alloc(std::max<size_t>(S, 1)));
  HIPCHK(c, dlevel.alloc(std::max<size_t>(S, 1)));
  if (S > 0) {
    HIPCHK(c, hipMemcpyAsync(dpos.p, pos, S * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(dgs.p, gene_start, S * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(dge.p, gene_end, S * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(dflags.p, flags, S, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(dcode.p, code, S, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(dlevel.p, level, S * 8, hipMemcpyHostToDevice, c->stream));
  }
  return windows_build_dev(h, p, site_offset, dpos.p, dgs.p, dge.p, dflags.p, dcode.p, dlevel.p);
}

// ... from HOST site fields with the gene of every site chosen on the device (abn_genes.hip) in between
static int windows_build_sites(abn_windows* h, const abn_windows_params* p, abn_genes* genes, const abn_gene_rule* rule,
                               const int64_t* site_offset, const int32_t* chromosome, const uint32_t* start,
                               const uint32_t* end, const uint8_t* strand, const uint8_t* code, const double* level) {
  abn_ctx* c = h->ctx;
  const size_t S = (size_t)site_offset[h->n];
  DevBuf<int32_t> dchrom;
  DevBuf<uint32_t> dstart, dend, dgs, dge;
  DevBuf<uint8_t> dstrand, dflags, dcode;
  DevBuf<double> dlevel;
  HIPCHK(c, dchrom.alloc(S));
  HIPCHK(c, dstart.alloc(S));
  HIPCHK(c, dend.alloc(S));
  HIPCHK(c, dstrand.alloc(S));
  HIPCHK(c, dgs.alloc(S));
  HIPCHK(c, dge.alloc(S));
  HIPCHK(c, dflags.alloc(S));
  HIPCHK(c, dcode.alloc(std::max<size_t>(S, 1)));
  HIPCHK(c, dlevel.alloc(std::max<size_t>(S, 1)));
  if (S > 0) {
    HIPCHK(c, hipMemcpyAsync(dchrom.p, chromosome, S * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(dstart.p, start, S * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(dend.p, end, S * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(dstrand.p, strand, S, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(dcode.p, code, S, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(dlevel.p, level, S * 8, hipMemcpyHostToDevice, c->stream));
  }
  if (int rc = genes_choose_dev(genes, rule, h->n, site_offset, dchrom.p, dstart.p, dend.p, dstrand.p, dgs.p, dge.p,
                                dflags.p, nullptr))
    return rc;
  return windows_build_dev(h, p, site_offset, dstart.p, dgs.p, dge.p, dflags.p, dcode.p, dlevel.p);
}

// ... from RESIDENT parse results (abn_sites_parse_dev, abn_sites_insert): every sample's records and inserted lines
// merged in file order straight into the arrays the gene choice and the placement read (abn_sites_merge.hpp); with
// `align`, the sites every sample shares (abn_sites_common.hpp; kAlignPosition) or the union of the samples' sites with
// filtered placeholders (abn_sites_union.hpp; kAlignUnion) gathered out of them first
static int windows_build_parsed(abn_windows* h, const abn_windows_params* p, abn_genes* genes, const abn_gene_rule* rule,
                                double filter, abn_sites* const* samples, int align) {
  abn_ctx* c = h->ctx;
  const int n = h->n;
  // the prologue: every sample merged with its keys, the two passes timed into merge_ms (no site at all: no event); the
  // gene arrays and the flags beside the merged arrays
  MergedSites m;
  DevBuf<uint32_t> dgs, dge;
  DevBuf<uint8_t> dflags;
  if (int rc = m.alloc(c, n, h->report.before.data())) return rc;
  const size_t S = (size_t)m.off[(size_t)n];
  HIPCHK(c, dgs.alloc(S));
  HIPCHK(c, dge.alloc(S));
  HIPCHK(c, dflags.alloc(S));
  Events<3> ev;
  if (S > 0) {
    if (int rc = ev.create(c)) return rc;
    if (int rc = m.merge_keyed(c, samples, filter, ev.e)) return rc;
  }
  // what the gene choice and the placement read: the merged arrays, or their aligned copies (n_common sites per sample;
  // the gene arrays and the flags, written behind the step, are the merged arrays' own: no longer than those; n_union
  // sites per sample: the gene arrays and the flags are allocated again)
  const int64_t* offset = m.off.data();
  const int32_t* chrom = m.chrom.p;
  const uint32_t *start = m.start.p, *end = m.end.p;
  const uint8_t *strand = m.strand.p, *code = m.code.p;
  const double* level = m.level.p;
  SiteKeys akey;
  DevBuf<uint8_t> acode;
  DevBuf<double> alevel;
  std::vector<int64_t> aligned_offset((size_t)n + 1, 0);
  if (align) {  // (no site at all: n_common = 0 through the same path)
    Alignment a;
    if (int rc = sites_align(c, align, n, offset, m.keys(), a)) return rc;
    const size_t A = (size_t)n * (size_t)a.each;
    if (int rc = akey.alloc(c, A)) return rc;
    HIPCHK(c, acode.alloc(std::max<size_t>(A, 1)));
    HIPCHK(c, alevel.alloc(std::max<size_t>(A, 1)));
    const CommonGather g{m.code.p, m.level.p, akey.chrom.p, akey.start.p, akey.end.p, akey.strand.p, alevel.p, acode.p, a.each};
    if (int rc = sites_align_gather(c, a, g)) return rc;
    sites_align_report(a, h->report);
    // A > S under the union alone (n_common is at most the shortest sample), and only this builder has arrays sized by
    // the merged sites that are written behind the step (the gather is complete: the merged arrays' gene arrays and
    // flags have no reader)
    if (A > S) {
      HIPCHK(c, dgs.alloc(A));
      HIPCHK(c, dge.alloc(A));
      HIPCHK(c, dflags.alloc(A));
    }
    for (int s = 0; s <= n; ++s) aligned_offset[(size_t)s] = (int64_t)s * a.each;
    offset = aligned_offset.data();
    chrom = akey.chrom.p, start = akey.start.p, end = akey.end.p, strand = akey.strand.p, code = acode.p, level = alevel.p;
  }
  // the builder's own: the gene choice and the placement
  if (offset[n] > 0)
    if (int rc = genes_choose_dev(genes, rule, n, offset, chrom, start, end, strand, dgs.p, dge.p, dflags.p, nullptr))
      return rc;  // (ends in a synchronisation)
  if (S > 0)
    for (int k = 0; k < 2; ++k)
      if (int rc = ev.elapsed_ms(c, k, &h->merge_ms[k])) return rc;
  return windows_build_dev(h, p, offset, start, dgs.p, dge.p, dflags.p, code, level);
}

// the checks of abn_windows_create and abn_windows_create_sites on what they share
static int windows_check(abn_ctx* c, const abn_windows_params* p, int32_t n_samples, const int64_t* site_offset,
                         abn_windows** out) {
  if (!p || !out || !site_offset || n_samples <= 0) return set_err(c, ABN_ERR_INVALID_ARG, "null/size");
  if (n_samples > 65535) return set_err(c, ABN_ERR_INVALID_ARG, "too many samples");
  if (p->step == 0) return set_err(c, ABN_ERR_INVALID_ARG, "window step 0");
  if (p->n_upstream < 0 || p->n_gene < 0 || p->n_downstream < 0 ||
      (long long)p->n_upstream + p->n_gene + p->n_downstream > (1 << 20))
    return set_err(c, ABN_ERR_INVALID_ARG, "window counts");
  return site_offset_check(c, n_samples, site_offset);
}

// the handle around build(handle): created, built, handed out
template <class Build>
static int windows_make(abn_ctx* c, const abn_windows_params* p, int32_t n_samples, const int64_t* site_offset,
                        abn_windows** out, Build build) {
  return handle_create(c, n_samples, out, [&](abn_windows* h) {
    h->W = p->n_upstream + p->n_gene + p->n_downstream;
    h->report.before.resize((size_t)n_samples);
    for (int s = 0; s < n_samples; ++s) h->report.before[(size_t)s] = site_offset[s + 1] - site_offset[s];
    return build(h);
  });
}

extern "C" int abn_windows_create_sites(abn_ctx* c, const abn_windows_params* p, abn_genes* genes, const abn_gene_rule* rule,
                                        int32_t n_samples, const int64_t* site_offset, const int32_t* chromosome,
                                        const uint32_t* start, const uint32_t* end, const uint8_t* strand,
                                        const uint8_t* code, const double* level, abn_windows** out) {
  if (!c) return ABN_ERR_INVALID_ARG;
  if (out) *out = nullptr;
  if (int rc = windows_check(c, p, n_samples, site_offset, out)) return rc;
  if (!genes || !rule) return set_err(c, ABN_ERR_INVALID_ARG, "null/size");
  if (genes_ctx(genes) != c) return set_err(c, ABN_ERR_INVALID_ARG, "the genes belong to another context");
  const int64_t S = site_offset[n_samples];
  if (S > 0 && (!chromosome || !start || !end || !strand || !code || !level))
    return set_err(c, ABN_ERR_INVALID_ARG, "null site arrays");
  for (int64_t i = 0; i < S; ++i)
    if (chromosome[i] < 0 || chromosome[i] >= 258 || strand[i] > 2)  // the table of abn_genes.hpp: 258 chromosome keys
      return set_err(c, ABN_ERR_INVALID_ARG, "a site's chromosome is outside 0..257, or its strand above 2");
  return windows_make(c, p, n_samples, site_offset, out, [&](abn_windows* h) {
    return windows_build_sites(h, p, genes, rule, site_offset, chromosome, start, end, strand, code, level);
  });
}

static int windows_create_parsed(abn_ctx* c, const abn_windows_params* p, abn_genes* genes, const abn_gene_rule* rule,
                                 double posterior_max_filter, int32_t n_samples, abn_sites* const* samples, int align,
                                 abn_windows** out) {
  if (!c) return ABN_ERR_INVALID_ARG;
  if (out) *out = nullptr;
  if (!p || !out || !samples || n_samples <= 0) return set_err(c, ABN_ERR_INVALID_ARG, "null/size");
  if (n_samples > 65535) return set_err(c, ABN_ERR_INVALID_ARG, "too many samples");
  std::vector<int64_t> site_offset;
  try {
    site_offset.assign((size_t)n_samples + 1, 0);
  } catch (const std::bad_alloc&) {
    return set_err(c, ABN_ERR_HIP, "out of host memory");
  }
  if (int rc = resident_counts(c, n_samples, samples, site_offset.data() + 1)) return rc;
  for (int s = 0; s < n_samples; ++s) site_offset[(size_t)s + 1] += site_offset[(size_t)s];
  if (int rc = windows_check(c, p, n_samples, site_offset.data(), out)) return rc;
  if (!genes || !rule) return set_err(c, ABN_ERR_INVALID_ARG, "null/size");
  if (genes_ctx(genes) != c) return set_err(c, ABN_ERR_INVALID_ARG, "the genes belong to another context");
  return windows_make(c, p, n_samples, site_offset.data(), out, [&](abn_windows* h) {
    return windows_build_parsed(h, p, genes, rule, posterior_max_filter, samples, align);
  });
}

extern "C" int abn_windows_create_parsed(abn_ctx* c, const abn_windows_params* p, abn_genes* genes,
                                         const abn_gene_rule* rule, double posterior_max_filter, int32_t n_samples,
                                         abn_sites* const* samples, abn_windows** out) {
  return windows_create_parsed(c, p, genes, rule, posterior_max_filter, n_samples, samples, kAlignNone, out);
}

extern "C" int abn_windows_create_aligned(abn_ctx* c, const abn_windows_params* p, abn_genes* genes,
                                          const abn_gene_rule* rule, double posterior_max_filter, int32_t n_samples,
                                          abn_sites* const* samples, abn_windows** out) {
  return windows_create_parsed(c, p, genes, rule, posterior_max_filter, n_samples, samples, kAlignPosition, out);
}

extern "C" int abn_windows_create_union(abn_ctx* c, const abn_windows_params* p, abn_genes* genes,
                                        const abn_gene_rule* rule, double posterior_max_filter, int32_t n_samples,
                                        abn_sites* const* samples, abn_windows** out) {
  return windows_create_parsed(c, p, genes, rule, posterior_max_filter, n_samples, samples, kAlignUnion, out);
}

extern "C" int abn_windows_create(abn_ctx* c, const abn_windows_params* p, int32_t n_samples, const int64_t* site_offset,
                                  const uint32_t* pos, const uint32_t* gene_start, const uint32_t* gene_end,
                                  const uint8_t* flags, const uint8_t* code, const double* level, abn_windows** out) {
  if (!c) return ABN_ERR_INVALID_ARG;
  if (out) *out = nullptr;
  if (int rc = windows_check(c, p, n_samples, site_offset, out)) return rc;
  if (site_offset[n_samples] > 0 && (!pos || !gene_start || !gene_end || !flags || !code || !level))
    return set_err(c, ABN_ERR_INVALID_ARG, "null site arrays");
  return windows_make(c, p, n_samples, site_offset, out, [&](abn_windows* h) {
    return windows_build(h, p, site_offset, pos, gene_start, gene_end, flags, code, level);
  });
}

extern "C" int abn_windows_destroy(abn_windows* h) { return handle_destroy(h); }

extern "C" int abn_windows_info(const abn_windows* h, int32_t* n_windows, int64_t* row_stride, int64_t* n_sites) {
  if (!h) return ABN_ERR_INVALID_ARG;
  if (n_windows) *n_windows = h->W;
  if (row_stride) *row_stride = h->stride;
  if (n_sites) *n_sites = 4 * h->stride;
  return ABN_OK;
}

extern "C" int abn_windows_merge_ms(const abn_windows* h, double* ms2) {
  if (!h || !ms2) return ABN_ERR_INVALID_ARG;
  ms2[0] = h->merge_ms[0];
  ms2[1] = h->merge_ms[1];
  return ABN_OK;
}

extern "C" int abn_windows_common(const abn_windows* h, int64_t* before, int64_t* n_common, double* ms4) {
  return h ? h->report.common(before, n_common, ms4) : ABN_ERR_INVALID_ARG;
}

extern "C" int abn_windows_union(const abn_windows* h, int64_t* before, int64_t* n_union, double* ms8) {
  return h ? h->report.unite(before, n_union, ms8) : ABN_ERR_INVALID_ARG;
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

extern "C" int abn_windows_packed(abn_windows* h, uint8_t* host_out) { return handle_packed(h, host_out); }

extern "C" int abn_windows_pairwise(abn_windows* h, uint64_t* diff, uint64_t* both, double* dvalue) {
  if (!h) return ABN_ERR_INVALID_ARG;
  abn_ctx* c = h->ctx;
  const size_t n = (size_t)h->n, nout = n * (n - 1) / 2 * (size_t)h->W;
  if (nout == 0) return ABN_OK;
  HIPCHK(c, hipSetDevice(c->device));
  PoolScope pool_scope(c);
  return pairwise_to_host(c, nout, diff, both, dvalue, [&](auto* dd, auto* db, auto* dv) {
    return pairwise_windows_packed_dev(c, h->packed.p, h->n, 4 * h->stride, h->stride, h->begin.data(), h->end.data(),
                                       h->W, dd, db, dv, nullptr);
  });
}
