// abn_genes_*: the annotation resident on the device and the choice of a gene per site.  Kernels: abn_genes.hpp;
// abn_windows_create_sites (abn_windows.hip) feeds the choice straight into the window placement.
#include "abn_host.hpp"

#define ABN_GENES_KERNELS
#include "abn_genes.hpp"

using namespace abn;

struct abn_genes {
  abn_ctx* ctx = nullptr;
  DevBuf<uint32_t> list_offset, list_count, start, end;  // the table [258 x 3]; the flattened genes
  DevBuf<uint16_t> chromosome;
  DevBuf<uint8_t> strand;
  GeneTable table() const { return GeneTable{list_offset.p, list_count.p, chromosome.p, start.p, end.p, strand.p}; }
};

abn_ctx* abn::genes_ctx(const abn_genes* h) { return h ? h->ctx : nullptr; }

static int genes_upload(abn_genes* h, int32_t n_lists, const int32_t* list_chromosome, const int32_t* list_kind,
                        const int64_t* list_offset, const uint32_t* gene_start, const uint32_t* gene_end,
                        const uint8_t* gene_strand) {
  abn_ctx* c = h->ctx;
  const size_t G = (size_t)list_offset[n_lists], cells = (size_t)kGeneChromosomes * kGeneKinds;
  std::vector<uint32_t> off(cells, 0), cnt(cells, 0);
  std::vector<uint16_t> chrom(G);
  for (int l = 0; l < n_lists; ++l) {
    const size_t cell = (size_t)list_chromosome[l] * kGeneKinds + (size_t)list_kind[l];
    off[cell] = (uint32_t)list_offset[l];
    cnt[cell] = (uint32_t)(list_offset[l + 1] - list_offset[l]);
    for (int64_t g = list_offset[l]; g < list_offset[l + 1]; ++g) chrom[(size_t)g] = (uint16_t)list_chromosome[l];
  }
  int rc;
  if ((rc = upload(c, h->list_offset, off.data(), cells)) || (rc = upload(c, h->list_count, cnt.data(), cells))) return rc;
  HIPCHK(c, h->start.alloc(std::max<size_t>(G, 1)));  // (at least one element each, so that no pointer is null)
  HIPCHK(c, h->end.alloc(std::max<size_t>(G, 1)));
  HIPCHK(c, h->chromosome.alloc(std::max<size_t>(G, 1)));
  HIPCHK(c, h->strand.alloc(std::max<size_t>(G, 1)));
  if (G > 0 && ((rc = to_device(c, h->start.p, gene_start, G * 4)) || (rc = to_device(c, h->end.p, gene_end, G * 4)) ||
                (rc = to_device(c, h->chromosome.p, chrom.data(), G * 2)) || (rc = to_device(c, h->strand.p, gene_strand, G))))
    return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));  // the staging vectors go on return
  return ABN_OK;
}

extern "C" int abn_genes_create(abn_ctx* c, int32_t n_lists, const int32_t* list_chromosome, const int32_t* list_kind,
                                const int64_t* list_offset, const uint32_t* gene_start, const uint32_t* gene_end,
                                const uint8_t* gene_strand, abn_genes** out) {
  if (!c) return ABN_ERR_INVALID_ARG;
  if (out) *out = nullptr;
  if (!out || !list_offset || n_lists < 0 || (n_lists > 0 && (!list_chromosome || !list_kind)))
    return set_err(c, ABN_ERR_INVALID_ARG, "null/size");
  if (list_offset[0] != 0) return set_err(c, ABN_ERR_INVALID_ARG, "list_offset[0] is not 0");
  try {
    std::vector<char> seen((size_t)kGeneChromosomes * kGeneKinds, 0);
    for (int l = 0; l < n_lists; ++l) {
      if (list_chromosome[l] < 0 || list_chromosome[l] >= kGeneChromosomes)
        return set_err(c, ABN_ERR_INVALID_ARG, "a list's chromosome is outside 0..257");
      if (list_kind[l] < 0 || list_kind[l] >= kGeneKinds) return set_err(c, ABN_ERR_INVALID_ARG, "a list's kind is outside 0..2");
      char& s = seen[(size_t)list_chromosome[l] * kGeneKinds + (size_t)list_kind[l]];
      if (s) return set_err(c, ABN_ERR_INVALID_ARG, "a (chromosome, kind) list is given twice");
      s = 1;
      if (list_offset[l + 1] < list_offset[l] || list_offset[l + 1] > 0xfffffffeLL)
        return set_err(c, ABN_ERR_INVALID_ARG, "list_offset is not ascending, or 2^32 - 1 genes or more");
    }
    const int64_t G = list_offset[n_lists];
    if (G > 0 && (!gene_start || !gene_end || !gene_strand)) return set_err(c, ABN_ERR_INVALID_ARG, "null gene arrays");
    for (int64_t g = 0; g < G; ++g)
      if (gene_strand[g] > 2) return set_err(c, ABN_ERR_INVALID_ARG, "a gene's strand is above 2");
    HIPCHK(c, hipSetDevice(c->device));
    std::unique_ptr<abn_genes> h(new abn_genes);  // its buffers live as long as the handle: not drawn from the pool
    h->ctx = c;
    if (int rc = genes_upload(h.get(), n_lists, list_chromosome, list_kind, list_offset, gene_start, gene_end, gene_strand))
      return rc;
    *out = h.release();
  } catch (const std::bad_alloc&) {
    return set_err(c, ABN_ERR_HIP, "out of host memory");
  }
  return ABN_OK;
}

extern "C" int abn_genes_destroy(abn_genes* h) {
  if (!h) return ABN_ERR_INVALID_ARG;
  (void)hipSetDevice(h->ctx->device);
  delete h;
  return ABN_OK;
}

// the checks both forms share; *n_sites = site_offset[n_samples]
static int genes_check(abn_genes* h, const abn_gene_rule* rule, int32_t n_samples, const int64_t* site_offset,
                       int64_t* n_sites) {
  abn_ctx* c = h->ctx;
  if (!rule || !site_offset || n_samples <= 0) return set_err(c, ABN_ERR_INVALID_ARG, "null/size");
  if (n_samples > 65535) return set_err(c, ABN_ERR_INVALID_ARG, "too many samples");
  if (int rc = site_offset_check(c, n_samples, site_offset)) return rc;
  if ((site_offset[n_samples] + kGeneBlockSites - 1) / kGeneBlockSites + n_samples > 0x7fffffffLL)
    return set_err(c, ABN_ERR_INVALID_ARG, "too many sites for one call");
  *n_sites = site_offset[n_samples];
  return ABN_OK;
}

int abn::genes_choose_dev(abn_genes* h, const abn_gene_rule* rule, int32_t n_samples, const int64_t* site_offset,
                          const int32_t* dchrom, const uint32_t* dstart, const uint32_t* dend, const uint8_t* dstrand,
                          uint32_t* dgene_start, uint32_t* dgene_end, uint8_t* dflags, double* kernel_ms) {
  if (!h) return ABN_ERR_INVALID_ARG;
  abn_ctx* c = h->ctx;
  int64_t S = 0;
  if (int rc = genes_check(h, rule, n_samples, site_offset, &S)) return rc;
  if (kernel_ms) kernel_ms[0] = kernel_ms[1] = kernel_ms[2] = 0.0;
  if (S == 0) return ABN_OK;
  if (!dchrom || !dstart || !dend || !dstrand || !dgene_start || !dgene_end || !dflags)
    return set_err(c, ABN_ERR_INVALID_ARG, "null site arrays");
  const int n = n_samples;
  // the blocks: kGeneBlockSites sites each, never across two samples
  std::vector<GeneBlock> blocks;
  std::vector<int> block0((size_t)n + 1, 0);
  for (int s = 0; s < n; ++s) {
    for (long long b = site_offset[s]; b < site_offset[s + 1]; b += kGeneBlockSites)
      blocks.push_back(GeneBlock{b, (int)std::min<long long>(kGeneBlockSites, site_offset[s + 1] - b), s});
    block0[(size_t)s + 1] = (int)blocks.size();
  }
  const size_t NB = blocks.size();
  DevBuf<GeneBlock> dblocks;
  DevBuf<int> dblock0, dbad;
  DevBuf<uint32_t> dF, dcarry;
  DevBuf<uint16_t> dnext, dlast, dentry;
  if (int rc = upload(c, dblocks, blocks.data(), NB)) return rc;
  if (int rc = upload(c, dblock0, block0.data(), (size_t)n + 1)) return rc;
  HIPCHK(c, dbad.alloc((size_t)n));
  HIPCHK(c, dF.alloc((size_t)S));
  HIPCHK(c, dnext.alloc((size_t)S));
  HIPCHK(c, dlast.alloc((size_t)S));
  HIPCHK(c, dentry.alloc(NB));
  HIPCHK(c, dcarry.alloc(NB));
  Events<4> ev;
  if (kernel_ms)
    if (int rc = ev.create(c)) return rc;
  auto mark = [&](int k) { return kernel_ms ? ev.record(c, k) : ABN_OK; };
  const GeneSites sites{dchrom, dstart, dend, dstrand};
  const GeneTable table = h->table();
  const GeneRule r{rule->cutoff, rule->cutoff_gene_length};
  if (int rc = mark(0)) return rc;
  hipLaunchKernelGGL(abn_genes_find_kernel, dim3((unsigned)NB), dim3(kGeneThreads), 0, c->stream, sites, dblocks.p, table,
                     r, dF.p, dnext.p, dlast.p);
  HIPCHK(c, hipGetLastError());
  if (int rc = mark(1)) return rc;
  hipLaunchKernelGGL(abn_genes_carry_kernel, dim3((unsigned)n), dim3(kGeneThreads), 0, c->stream, sites, dblocks.p,
                     dblock0.p, table, r, dF.p, dlast.p, dentry.p, dcarry.p, dbad.p);
  HIPCHK(c, hipGetLastError());
  if (int rc = mark(2)) return rc;
  hipLaunchKernelGGL(abn_genes_write_kernel, dim3((unsigned)NB), dim3(kGeneThreads), 0, c->stream, sites, dblocks.p, table,
                     dF.p, dnext.p, dentry.p, dcarry.p, dgene_start, dgene_end, dflags);
  HIPCHK(c, hipGetLastError());
  if (int rc = mark(3)) return rc;
  std::vector<int> bad((size_t)n, 0);
  if (int rc = to_host(c, bad.data(), dbad)) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));  // the scratch buffers are freed on return
  if (kernel_ms)
    for (int k = 0; k < 3; ++k)
      if (int rc = ev.elapsed_ms(c, k, &kernel_ms[k])) return rc;
  for (int s = 0; s < n; ++s)
    if (bad[(size_t)s]) return set_err(c, ABN_ERR_INVALID_ARG, "a site's chromosome is outside 0..257, or its strand above 2");
  return ABN_OK;
}

extern "C" int abn_genes_choose_dev(abn_genes* h, const abn_gene_rule* rule, int32_t n_samples, const int64_t* site_offset,
                                    const void* dev_chromosome, const void* dev_start, const void* dev_end,
                                    const void* dev_strand, void* dev_gene_start, void* dev_gene_end, void* dev_flags,
                                    double* kernel_ms) {
  if (!h) return ABN_ERR_INVALID_ARG;
  abn_ctx* c = h->ctx;
  HIPCHK(c, hipSetDevice(c->device));
  PoolScope pool_scope(c);
  try {
    return genes_choose_dev(h, rule, n_samples, site_offset, (const int32_t*)dev_chromosome, (const uint32_t*)dev_start,
                            (const uint32_t*)dev_end, (const uint8_t*)dev_strand, (uint32_t*)dev_gene_start,
                            (uint32_t*)dev_gene_end, (uint8_t*)dev_flags, kernel_ms);
  } catch (const std::bad_alloc&) {
    return set_err(c, ABN_ERR_HIP, "out of host memory");
  }
}

extern "C" int abn_genes_choose(abn_genes* h, const abn_gene_rule* rule, int32_t n_samples, const int64_t* site_offset,
                                const int32_t* chromosome, const uint32_t* start, const uint32_t* end,
                                const uint8_t* strand, uint32_t* gene_start, uint32_t* gene_end, uint8_t* flags,
                                double* kernel_ms) {
  if (!h) return ABN_ERR_INVALID_ARG;
  abn_ctx* c = h->ctx;
  int64_t n_sites = 0;
  if (int rc = genes_check(h, rule, n_samples, site_offset, &n_sites)) return rc;
  const size_t S = (size_t)n_sites;
  if (kernel_ms) kernel_ms[0] = kernel_ms[1] = kernel_ms[2] = 0.0;
  if (S == 0) return ABN_OK;
  if (!chromosome || !start || !end || !strand || !gene_start || !gene_end || !flags)
    return set_err(c, ABN_ERR_INVALID_ARG, "null site arrays");
  for (size_t i = 0; i < S; ++i)
    if (chromosome[i] < 0 || chromosome[i] >= kGeneChromosomes || strand[i] > 2)
      return set_err(c, ABN_ERR_INVALID_ARG, "a site's chromosome is outside 0..257, or its strand above 2");
  HIPCHK(c, hipSetDevice(c->device));
  PoolScope pool_scope(c);
  DevBuf<int32_t> dchrom;
  DevBuf<uint32_t> dstart, dend, dgs, dge;
  DevBuf<uint8_t> dstrand, dflags;
  int rc;
  if ((rc = upload(c, dchrom, chromosome, S)) || (rc = upload(c, dstart, start, S)) || (rc = upload(c, dend, end, S)) ||
      (rc = upload(c, dstrand, strand, S)))
    return rc;
  HIPCHK(c, dgs.alloc(S));
  HIPCHK(c, dge.alloc(S));
  HIPCHK(c, dflags.alloc(S));
  try {
    if ((rc = genes_choose_dev(h, rule, n_samples, site_offset, dchrom.p, dstart.p, dend.p, dstrand.p, dgs.p, dge.p,
                               dflags.p, kernel_ms)))
      return rc;
  } catch (const std::bad_alloc&) {
    return set_err(c, ABN_ERR_HIP, "out of host memory");
  }
  if ((rc = to_host(c, gene_start, dgs)) || (rc = to_host(c, gene_end, dge)) || (rc = to_host(c, flags, dflags))) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return ABN_OK;
}
