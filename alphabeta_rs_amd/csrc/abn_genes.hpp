// The choice of a gene per methylome site (abn_genes_*): the loop of Windows::extract (src/windows.rs:325-338) around
// is_in_gene / find_gene (src/methylation_site.rs:368-418) with its last_gene cache, without the serial dependence.
//
//   in(s, g)   is_in_gene: u32 arithmetic that wraps, chromosome equality, Strand::eq
//   F_i        find_gene(s_i): slice::binary_search_by probe for probe, then is_in_gene; a gene or none; site i alone
//   the loop   miss_i = state_{i-1} is none or !in(s_i, state_{i-1});  state_i = miss_i ? F_i : state_{i-1};
//              none in front of every sample's first site
//
// Every sample is cut into blocks of B sites (never across two samples).  For a miss at k, next(k) is the next miss of
// its block: k + 1 when F_k is none, else the first j > k of the block with !in(s_j, F_k), END when there is none.
// last(k) is the last miss on the chain k -> next(k) -> ...
//
//   G1 abn_genes_find_kernel    every block alone: F, next and last of every site (last by pointer jumping)
//   G2 abn_genes_carry_kernel   a workgroup per sample, serial over its blocks: with carry-in g the block's entry e is its
//                               first site when g is none, else the first j with !in(s_j, g), else END (a workgroup-wide
//                               min); carry-out F[last(e)], or g when e is END; (e, g) written per block
//   G3 abn_genes_write_kernel   every block alone: the chain from e marks the misses; a site takes the F of the latest
//                               miss at or before it, the carry-in in front of e -> gene_start, gene_end, flags
// Every output element has exactly one writer and is written with a plain vector store; there are no atomics, no kernel
// waits for another workgroup, every loop is bounded by the block length or the sample's block count.
//
// The arithmetic and the three phases in their serial form (any block length up to 65534) compile without a HIP header:
// the host library (host_capi.cpp) and tests/native/genes_blocks_main.cpp include this file as it is.
#pragma once
#include <stdint.h>

#ifndef ABN_HOST_DEVICE
#if defined(__HIPCC__) || defined(__CUDACC__)
#define ABN_HOST_DEVICE __host__ __device__
#else
#define ABN_HOST_DEVICE
#endif
#endif

namespace abn {

constexpr int kGeneChromosomes = 258;  // Numbered(0..255), Mitochondrial = 256, Chloroplast = 257
constexpr int kGeneKinds = 3;          // the lists of GenesByStrand: sense, antisense, combined — a site's strand picks one
constexpr uint32_t kGeneNone = 0xffffffffu;
constexpr uint16_t kGeneEnd = 0xffffu;  // END: no further miss in the block
constexpr int kGeneThreads = 256;
constexpr int kGeneBlockSites = 1024;  // = kWinBlockSites; G1 holds a block's fields (13 KiB) and its chain (2 KiB) in LDS
constexpr int kGenePer = kGeneBlockSites / kGeneThreads;

struct GeneRule {  // abn_gene_rule
  uint32_t cutoff;
  int32_t cutoff_gene_length;
};

struct GeneTable {  // the annotation: list (chromosome, kind) = genes [offset, offset + count) of the flattened arrays
  const uint32_t* list_offset;  // [kGeneChromosomes x kGeneKinds]
  const uint32_t* list_count;
  const uint16_t* chromosome;  // per gene
  const uint32_t* start;
  const uint32_t* end;
  const uint8_t* strand;  // 0 Sense, 1 Antisense, 2 Unknown
};

struct GeneSites {  // struct-of-arrays, file order
  const int32_t* chromosome;
  const uint32_t* start;
  const uint32_t* end;
  const uint8_t* strand;
};

struct GeneBlock {  // sites [site0, site0 + len) of `sample`
  long long site0;
  int len, sample;
};

// Strand::eq (src/genes.rs:88-96): Unknown equals both
ABN_HOST_DEVICE inline bool gene_strand_eq(uint32_t a, uint32_t b) { return !((a == 0 && b == 1) || (a == 1 && b == 0)); }

// is_in_gene (src/methylation_site.rs:368-378) of site i and gene g
ABN_HOST_DEVICE inline bool gene_in(const GeneSites& S, long long i, const GeneTable& T, uint32_t g, const GeneRule& r) {
  const uint32_t gs = T.start[g], ge = T.end[g];
  const uint32_t cutoff = r.cutoff_gene_length ? ge - gs : r.cutoff;
  return S.chromosome[i] == (int32_t)T.chromosome[g] && gs <= S.start[i] + cutoff && S.end[i] <= ge + cutoff &&
         gene_strand_eq(S.strand[i], T.strand[g]);
}

// the key find_gene searches by (src/methylation_site.rs:395-403)
ABN_HOST_DEVICE inline uint32_t gene_key(const GeneTable& T, uint32_t g, const GeneRule& r) {
  return r.cutoff_gene_length ? T.end[g] + (T.end[g] - T.start[g]) : T.end[g] + r.cutoff;
}

// find_gene (src/methylation_site.rs:385-418) of site i: binary_search_by in its `size / 2` form over the list of the
// site's chromosome and strand, then is_in_gene.  A chromosome outside the table has no list.
ABN_HOST_DEVICE inline uint32_t gene_find(const GeneSites& S, long long i, const GeneTable& T, const GeneRule& r) {
  const int32_t c = S.chromosome[i];
  const uint32_t kind = S.strand[i];
  if (c < 0 || c >= kGeneChromosomes || kind >= (uint32_t)kGeneKinds) return kGeneNone;
  const uint32_t base = T.list_offset[c * kGeneKinds + (int)kind], n = T.list_count[c * kGeneKinds + (int)kind];
  const uint32_t target = S.start[i];
  uint32_t size = n, left = 0, right = n;
  while (left < right) {
    const uint32_t mid = left + size / 2;
    const uint32_t k = gene_key(T, base + mid, r);
    if (k == target) {
      left = mid;
      break;
    }
    if (k < target) left = mid + 1;
    else right = mid;
    size = right - left;
  }
  if (left >= n) return kGeneNone;
  return gene_in(S, i, T, base + left, r) ? base + left : kGeneNone;
}

// next(k) inside the block whose sites are S[0 .. len): S points at the block's first site
ABN_HOST_DEVICE inline uint16_t gene_next(const GeneSites& S, int k, int len, uint32_t Fk, const GeneTable& T,
                                          const GeneRule& r) {
  if (Fk == kGeneNone) return k + 1 < len ? (uint16_t)(k + 1) : kGeneEnd;
  for (int j = k + 1; j < len; ++j)
    if (!gene_in(S, j, T, Fk, r)) return (uint16_t)j;
  return kGeneEnd;
}

// what choose_gene pushes for a site with gene g (or none): flags bit 0 antisense site, bit 1 has a gene
ABN_HOST_DEVICE inline void gene_output(uint32_t site_strand, const GeneTable& T, uint32_t g, uint32_t& gene_start,
                                        uint32_t& gene_end, uint8_t& flags) {
  gene_start = g == kGeneNone ? 0u : T.start[g];
  gene_end = g == kGeneNone ? 0u : T.end[g];
  flags = (uint8_t)((site_strand == 1 ? 1u : 0u) | (g == kGeneNone ? 0u : 2u));
}

inline GeneSites gene_sites_at(const GeneSites& S, long long i) {
  return GeneSites{S.chromosome + i, S.start + i, S.end + i, S.strand + i};
}

// ---- the three phases, serial (the host form: any block length)
// G1 of one block: F, next, last [len] each
inline void genes_block_find(const GeneSites& B, int len, const GeneTable& T, const GeneRule& r, uint32_t* F,
                             uint16_t* next, uint16_t* last) {
  for (int k = 0; k < len; ++k) F[k] = gene_find(B, k, T, r);
  for (int k = 0; k < len; ++k) next[k] = gene_next(B, k, len, F[k], T, r);
  for (int k = len - 1; k >= 0; --k) last[k] = next[k] == kGeneEnd ? (uint16_t)k : last[next[k]];
}

// G2 of one block with carry-in g: its entry; returns the carry-out
inline uint32_t genes_block_carry(const GeneSites& B, int len, const GeneTable& T, const GeneRule& r, const uint32_t* F,
                                  const uint16_t* last, uint32_t g, uint16_t& entry) {
  entry = kGeneEnd;
  if (g == kGeneNone) entry = len > 0 ? 0 : kGeneEnd;
  else
    for (int j = 0; j < len && entry == kGeneEnd; ++j)
      if (!gene_in(B, j, T, g, r)) entry = (uint16_t)j;
  return entry == kGeneEnd ? g : F[last[entry]];
}

// G3 of one block: gene_start, gene_end, flags [len] each
inline void genes_block_write(const GeneSites& B, int len, const GeneTable& T, const uint32_t* F, const uint16_t* next,
                              uint16_t entry, uint32_t g, uint32_t* gene_start, uint32_t* gene_end, uint8_t* flags) {
  const int e = entry == kGeneEnd ? len : (int)entry;
  for (int k = 0; k < e; ++k) gene_output(B.strand[k], T, g, gene_start[k], gene_end[k], flags[k]);
  for (int m = e; m < len;) {
    const int stop = next[m] == kGeneEnd ? len : (int)next[m];
    for (int k = m; k < stop; ++k) gene_output(B.strand[k], T, F[m], gene_start[k], gene_end[k], flags[k]);
    m = stop;
  }
}

// all three over samples cut into blocks of block_sites (1 .. 65534) sites; the scratch arrays are the caller's: F, next,
// last [site_offset[n_samples]] each
inline void genes_choose_blocked(const GeneSites& S, const int64_t* site_offset, int n_samples, const GeneTable& T,
                                 const GeneRule& r, int block_sites, uint32_t* F, uint16_t* next, uint16_t* last,
                                 uint32_t* gene_start, uint32_t* gene_end, uint8_t* flags) {
  for (int s = 0; s < n_samples; ++s)
    for (long long b = site_offset[s]; b < site_offset[s + 1]; b += block_sites) {
      const int len = (int)(site_offset[s + 1] - b < block_sites ? site_offset[s + 1] - b : block_sites);
      genes_block_find(gene_sites_at(S, b), len, T, r, F + b, next + b, last + b);
    }
  for (int s = 0; s < n_samples; ++s) {
    uint32_t g = kGeneNone;
    for (long long b = site_offset[s]; b < site_offset[s + 1]; b += block_sites) {
      const int len = (int)(site_offset[s + 1] - b < block_sites ? site_offset[s + 1] - b : block_sites);
      uint16_t entry;
      const uint32_t out = genes_block_carry(gene_sites_at(S, b), len, T, r, F + b, last + b, g, entry);
      genes_block_write(gene_sites_at(S, b), len, T, F + b, next + b, entry, g, gene_start + b, gene_end + b, flags + b);
      g = out;
    }
  }
}

#ifdef ABN_GENES_KERNELS
// ---- the kernels (abn_genes.hip defines ABN_GENES_KERNELS and includes the HIP runtime in front of this file)
// G1.  A lane takes the sites t, t + 256, ..: the binary search reads the annotation from global memory (a few hundred
// genes per list: it stays in the caches), the forward search of next reads the block's fields from LDS, neighbouring
// lanes at neighbouring addresses.  last: ptr = next (a terminal site points at itself), ten rounds of ptr = ptr[ptr]
// cover chains of up to 1024 links.
__global__ void __launch_bounds__(kGeneThreads)
abn_genes_find_kernel(GeneSites S, const GeneBlock* __restrict__ blocks, GeneTable T, GeneRule rule,
                      uint32_t* __restrict__ F, uint16_t* __restrict__ next, uint16_t* __restrict__ last) {
  __shared__ int32_t s_chrom[kGeneBlockSites];
  __shared__ uint32_t s_start[kGeneBlockSites], s_end[kGeneBlockSites];
  __shared__ uint8_t s_strand[kGeneBlockSites];
  __shared__ uint16_t s_ptr[kGeneBlockSites];
  const GeneBlock blk = blocks[blockIdx.x];
  const int len = blk.len < kGeneBlockSites ? blk.len : kGeneBlockSites;
  for (int t = threadIdx.x; t < len; t += kGeneThreads) {
    s_chrom[t] = S.chromosome[blk.site0 + t];
    s_start[t] = S.start[blk.site0 + t];
    s_end[t] = S.end[blk.site0 + t];
    s_strand[t] = S.strand[blk.site0 + t];
  }
  __syncthreads();
  const GeneSites B{s_chrom, s_start, s_end, s_strand};
  for (int t = threadIdx.x; t < len; t += kGeneThreads) {
    const uint32_t f = gene_find(B, t, T, rule);
    F[blk.site0 + t] = f;
    const uint16_t nx = gene_next(B, t, len, f, T, rule);
    next[blk.site0 + t] = nx;
    s_ptr[t] = nx == kGeneEnd ? (uint16_t)t : nx;
  }
  __syncthreads();
  for (int round = 0; round < 10; ++round) {
    uint16_t p[kGenePer];
#pragma unroll
    for (int q = 0; q < kGenePer; ++q) {
      const int t = (int)threadIdx.x + q * kGeneThreads;
      p[q] = t < len ? s_ptr[s_ptr[t]] : (uint16_t)0;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < kGenePer; ++q) {
      const int t = (int)threadIdx.x + q * kGeneThreads;
      if (t < len) s_ptr[t] = p[q];
    }
    __syncthreads();
  }
  for (int t = threadIdx.x; t < len; t += kGeneThreads) last[blk.site0 + t] = s_ptr[t];
}

// G2.  The carry is the same value in every lane.  The block's fields do not depend on it: the next block's are loaded
// into registers in front of this block's reduction.  bad[sample] = 1: a site chromosome outside the table.
__global__ void __launch_bounds__(kGeneThreads)
abn_genes_carry_kernel(GeneSites S, const GeneBlock* __restrict__ blocks, const int* __restrict__ block0, GeneTable T,
                       GeneRule rule, const uint32_t* __restrict__ F, const uint16_t* __restrict__ last,
                       uint16_t* __restrict__ entry, uint32_t* __restrict__ carry, int* __restrict__ bad) {
  __shared__ int s_min[2][kGeneThreads / 64];
  __shared__ int s_bad[kGeneThreads / 64];
  const int sample = blockIdx.x, b_begin = block0[sample], b_end = block0[sample + 1];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t g = kGeneNone;
  int any_bad = 0;
  int32_t c[kGenePer] = {}, nc[kGenePer] = {};
  uint32_t a[kGenePer] = {}, z[kGenePer] = {}, na[kGenePer] = {}, nz[kGenePer] = {};
  uint8_t d[kGenePer] = {}, nd[kGenePer] = {};
  auto load = [&](int b, int32_t* pc, uint32_t* pa, uint32_t* pz, uint8_t* pd) {
    const GeneBlock blk = blocks[b];
#pragma unroll
    for (int q = 0; q < kGenePer; ++q) {
      const int t = (int)threadIdx.x + q * kGeneThreads;
      if (t < blk.len) {
        pc[q] = S.chromosome[blk.site0 + t];
        pa[q] = S.start[blk.site0 + t];
        pz[q] = S.end[blk.site0 + t];
        pd[q] = S.strand[blk.site0 + t];
      }
    }
  };
  if (b_begin < b_end) load(b_begin, nc, na, nz, nd);
  for (int b = b_begin; b < b_end; ++b) {
    const GeneBlock blk = blocks[b];
#pragma unroll
    for (int q = 0; q < kGenePer; ++q) c[q] = nc[q], a[q] = na[q], z[q] = nz[q], d[q] = nd[q];
    if (b + 1 < b_end) load(b + 1, nc, na, nz, nd);
    int e = 0x7fffffff;
    if (g == kGeneNone) {
      e = blk.len > 0 ? 0 : e;
    } else {
      const uint32_t gs = T.start[g], ge = T.end[g], gd = T.strand[g];
      const int32_t gc = (int32_t)T.chromosome[g];
      const uint32_t cutoff = rule.cutoff_gene_length ? ge - gs : rule.cutoff;
#pragma unroll
      for (int q = kGenePer - 1; q >= 0; --q) {
        const int t = (int)threadIdx.x + q * kGeneThreads;
        const bool in = c[q] == gc && gs <= a[q] + cutoff && z[q] <= ge + cutoff && gene_strand_eq(d[q], gd);
        if (t < blk.len && !in) e = t;
      }
    }
#pragma unroll
    for (int q = 0; q < kGenePer; ++q)
      if ((int)threadIdx.x + q * kGeneThreads < blk.len && (c[q] < 0 || c[q] >= kGeneChromosomes || d[q] > 2)) any_bad = 1;
    for (int off = 32; off > 0; off >>= 1) {
      const int o = __shfl_xor(e, off, 64);
      e = o < e ? o : e;
    }
    const int slot = (b - b_begin) & 1;  // two slots: a lane may run one block ahead of the slowest reader
    if (lane == 0) s_min[slot][wave] = e;
    __syncthreads();
#pragma unroll
    for (int w = 0; w < kGeneThreads / 64; ++w) e = s_min[slot][w] < e ? s_min[slot][w] : e;
    const uint32_t out = e == 0x7fffffff ? g : F[blk.site0 + last[blk.site0 + e]];
    if (threadIdx.x == 0) {
      entry[b] = e == 0x7fffffff ? kGeneEnd : (uint16_t)e;
      carry[b] = g;
    }
    g = out;
  }
  for (int off = 32; off > 0; off >>= 1) any_bad |= __shfl_xor(any_bad, off, 64);
  if (lane == 0) s_bad[wave] = any_bad;
  __syncthreads();
  if (threadIdx.x == 0) {
    int v = 0;
    for (int w = 0; w < kGeneThreads / 64; ++w) v |= s_bad[w];
    bad[sample] = v;
  }
}

// G3.  Lane 0 walks the chain from the entry and marks the misses (at most len steps); every lane then finds the latest
// miss at or before each of its four consecutive sites: its own sites first, else the latest of the lanes before it (a
// max-scan over the 256 lanes in LDS).
__global__ void __launch_bounds__(kGeneThreads)
abn_genes_write_kernel(GeneSites S, const GeneBlock* __restrict__ blocks, GeneTable T, const uint32_t* __restrict__ F,
                       const uint16_t* __restrict__ next, const uint16_t* __restrict__ entry,
                       const uint32_t* __restrict__ carry, uint32_t* __restrict__ gene_start,
                       uint32_t* __restrict__ gene_end, uint8_t* __restrict__ flags) {
  __shared__ uint16_t s_next[kGeneBlockSites];
  __shared__ uint8_t s_miss[kGeneBlockSites];
  __shared__ int s_scan[2][kGeneThreads];
  const GeneBlock blk = blocks[blockIdx.x];
  const int len = blk.len < kGeneBlockSites ? blk.len : kGeneBlockSites;
  const uint16_t e16 = entry[blockIdx.x];
  const uint32_t g = carry[blockIdx.x];
  for (int t = threadIdx.x; t < kGeneBlockSites; t += kGeneThreads) {
    s_next[t] = t < len ? next[blk.site0 + t] : kGeneEnd;
    s_miss[t] = 0;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int m = e16 == kGeneEnd ? len : (int)e16;
    for (int step = 0; step < len && m < len; ++step) {
      s_miss[m] = 1;
      const uint16_t nx = s_next[m];
      m = nx == kGeneEnd || (int)nx <= m ? len : (int)nx;
    }
  }
  __syncthreads();
  const int t0 = (int)threadIdx.x * kGenePer;
  int own = -1;
#pragma unroll
  for (int q = 0; q < kGenePer; ++q)
    if (s_miss[t0 + q]) own = t0 + q;
  s_scan[0][threadIdx.x] = own;
  __syncthreads();
  int src = 0;
  for (int off = 1; off < kGeneThreads; off <<= 1) {
    int v = s_scan[src][threadIdx.x];
    if ((int)threadIdx.x >= off) {
      const int o = s_scan[src][threadIdx.x - off];
      v = o > v ? o : v;
    }
    s_scan[src ^ 1][threadIdx.x] = v;
    src ^= 1;
    __syncthreads();
  }
  int latest = threadIdx.x > 0 ? s_scan[src][threadIdx.x - 1] : -1;
#pragma unroll
  for (int q = 0; q < kGenePer; ++q) {
    const int t = t0 + q;
    if (t >= len) break;
    if (s_miss[t]) latest = t;
    const uint32_t gene = latest < 0 ? g : F[blk.site0 + latest];
    uint32_t gs, ge;
    uint8_t fl;
    gene_output(S.strand[blk.site0 + t], T, gene, gs, ge, fl);
    gene_start[blk.site0 + t] = gs;
    gene_end[blk.site0 + t] = ge;
    flags[blk.site0 + t] = fl;
  }
}
#endif  // ABN_GENES_KERNELS

}  // namespace abn
