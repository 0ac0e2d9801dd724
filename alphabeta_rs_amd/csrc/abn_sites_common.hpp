// The sites every sample shares, by genomic position, on the device (abn_sites_common, abn_windows_create_aligned,
// abn_codes_create_aligned).  The reference compares site k of one methylome with site k of another and says so at
// src/pedigree.rs:240, "It is assumed that the same sites are included in the datasets"; this step lifts the assumption:
// it is an n-way intersection join of the samples' site arrays, after which position pairing is valid.
//
// A site's KEY is (chromosome, start, end, strand), the values abn_sites_fetch reports (chromosome 0..257, strand 0..2).
// The posterior and the status are no part of it: a filtered site is still a site.
//
// A sample is WELL ORDERED when every chromosome's sites form one contiguous run in file order and, inside a run,
// (start, end, strand) is strictly ascending (so no key occurs twice).  The runs may come in any order.  The COMMON SET is
// the set of keys present in every sample; every sample keeps its common sites in its own file order.  The samples are
// CO-ORDERED when the k-th common site of every sample has the same key, for every k.
//
// The samples' arrays lie one behind the other; sample s holds the sites [site_off[s], site_off[s + 1]).  The PROBE is the
// shortest sample (the lowest index among equals, common_pick_probe): its sites are looked up in every other sample.
//
//   runs    a lane per site: the first site of a run writes the run's begin into the table run_begin [n x 258] (an integer
//           atomicMin: with two runs of one chromosome the lower begin stays, whatever the arrival order); a site with its
//           predecessor's chromosome and a key not above the predecessor's records itself in err[kCommonNotAscending].
//   ends    a lane per site: the last site of a run writes run_end; the first site of a run that is not the table's begin
//           is the begin of a second run of its chromosome and records itself in err[kCommonSplitRun].  (Only in a sample
//           that is refused for it does run_end have two writers; its value is never used then.)
//   match   a lane per site of the probe: a lower bound of its key inside the run of its chromosome in every other sample,
//           kCommonSearches samples at a time so that as many independent loads are in flight, until a sample misses it.
//           keep = found in all; match[s][j] = where.  The workgroup's number of kept sites goes to block_count.
//   scan    one workgroup: the exclusive scan of block_count, the total (n_common) behind it.
//   rank    a lane per (sample, probe site): the kept site's rank k = its workgroup's offset + its rank in the workgroup;
//           src[s][k] = match[s][j].  Two levels, no workgroup waits for another.
//   gather  a lane per (sample, rank), after the host has read n_common: sample s's site src[s][k] is its k-th common site
//           if and only if src[s] ascends in k — the co-ordering check, with the key compared against the probe's at that
//           rank; a violation records the site in err[kCommonNotCoordered].  keep is set, and chromosome, start, end,
//           strand, code and level go to their aligned place.
//
// Every err entry is a lowest offending site index kept by an integer atomicMin, the only atomic here: few writers, and the
// result does not depend on their order.  Every other output element has one writer, a plain store.  A sample that is not
// well ordered still gives the searches in-bounds tables (begins and ends are indices of its own sites), so the match may
// run before the host looks at err.
//
// The comparator, the searches and the whole step in its serial form compile without a HIP header: the host library
// (host_capi.cpp) and tests/native/common_main.cpp include this file as it is.
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

#ifndef ABN_HOST_DEVICE
#if defined(__HIPCC__) || defined(__CUDACC__)
#define ABN_HOST_DEVICE __host__ __device__
#else
#define ABN_HOST_DEVICE
#endif
#endif

namespace abn {

constexpr int kCommonThreads = 256;
constexpr int kCommonChroms = 258;   // the chromosome keys of abn_sites_fetch: Numbered 0..255, Mitochondrial, Chloroplast
constexpr int kCommonSearches = 4;   // samples searched at a time by a lane of the match
constexpr long long kCommonNone = 0x7f7f7f7f7f7f7f7fLL;  // "no site": what a byte fill of 0x7f leaves; above every index

enum {  // the entries of err; as a refusal's kind, 0 is "none"
  kCommonSplitRun = 0,
  kCommonNotAscending = 1,
  kCommonBadKey = 2,  // a chromosome outside 0..257 or a strand above 2 (device arrays cannot be checked on the host)
  kCommonNotCoordered = 3,
  kCommonErrs = 4
};

struct CommonSites {  // the samples' key fields, one sample behind the other
  const int32_t* chromosome;
  const uint32_t* start;
  const uint32_t* end;
  const uint8_t* strand;
};

struct CommonKey {  // a key without its chromosome: what is ordered inside a run
  uint32_t start, end;
  uint32_t strand;
};

struct CommonGather {  // the gather's inputs and outputs beside the keys; every pointer may be null
  const uint8_t* code_in;  // at site_off, as the keys
  const double* level_in;
  int32_t* chromosome;  // sample s, rank k: at s * n_common + k
  uint32_t* start;
  uint32_t* end;
  uint8_t* strand;
  double* level;
  uint8_t* code;  // at s * code_stride + k
  long long code_stride;
};

struct CommonRefusal {  // kind: 1 + the err entry, 0 for none; site: the index inside the sample
  int kind;
  int sample;
  long long site;
};

ABN_HOST_DEVICE inline bool common_key_less(const CommonKey& a, const CommonKey& b) {
  if (a.start != b.start) return a.start < b.start;
  if (a.end != b.end) return a.end < b.end;
  return a.strand < b.strand;
}

ABN_HOST_DEVICE inline bool common_key_equal(const CommonKey& a, const CommonKey& b) {
  return a.start == b.start && a.end == b.end && a.strand == b.strand;
}

ABN_HOST_DEVICE inline CommonKey common_key_at(const CommonSites& a, long long i) {
  return CommonKey{a.start[i], a.end[i], (uint32_t)a.strand[i]};
}

ABN_HOST_DEVICE inline bool common_key_valid(int32_t chromosome, uint32_t strand) {
  return chromosome >= 0 && chromosome < kCommonChroms && strand <= 2u;
}

// *p = min(*p, v): the one atomic of the step
ABN_HOST_DEVICE inline void common_min(long long* p, long long v) {
#if defined(__HIP_DEVICE_COMPILE__)
  // (the compiler's builtin, what atomicMin is made of: this file compiles without a HIP header)
  (void)__hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
  if (v < *p) *p = v;
#endif
}

// the sample of site i: the last s with site_off[s] <= i (samples without a site are passed over)
ABN_HOST_DEVICE inline int common_sample_of(const long long* site_off, int n, long long i) {
  int lo = 0, hi = n;  // site_off[lo] <= i < site_off[hi]
  while (hi - lo > 1) {
    const int mid = lo + (hi - lo) / 2;
    if (site_off[mid] <= i) lo = mid;
    else hi = mid;
  }
  return lo;
}

// the shortest sample, the lowest index among equals
inline int common_pick_probe(const long long* site_off, int n) {
  int p = 0;
  for (int s = 1; s < n; ++s)
    if (site_off[s + 1] - site_off[s] < site_off[p + 1] - site_off[p]) p = s;
  return p;
}

// the first index of [lo, hi) whose key is not below `key` (hi if none): the lower bound inside one run
ABN_HOST_DEVICE inline long long common_lower_bound(const CommonSites& a, long long lo, long long hi, const CommonKey& key) {
  while (lo < hi) {
    const long long mid = lo + (hi - lo) / 2;
    if (common_key_less(common_key_at(a, mid), key)) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// The segmented search, for kCommonSearches samples at once: found[g] = the site of sample samples[g] (-1: no sample)
// with chromosome `chromosome` (valid) and key `key`, or -1.  The loads of a step are independent of one another; a search
// that is over reads the site `safe` (any valid index) and ignores it, so that no load sits under a branch.
ABN_HOST_DEVICE inline void common_find(const CommonSites& a, const long long* run_begin, const long long* run_end,
                                        const int samples[kCommonSearches], int chromosome, const CommonKey& key,
                                        long long safe, long long found[kCommonSearches]) {
  long long lo[kCommonSearches], hi[kCommonSearches], end[kCommonSearches];
  bool any = false;
  for (int g = 0; g < kCommonSearches; ++g) {
    lo[g] = hi[g] = end[g] = 0;
    if (samples[g] >= 0) {
      const long long at = (long long)samples[g] * kCommonChroms + chromosome;
      lo[g] = run_begin[at];
      hi[g] = end[g] = run_end[at];  // (a chromosome the sample lacks: begin kCommonNone, end 0)
    }
    any = any || lo[g] < hi[g];
  }
  while (any) {
    long long mid[kCommonSearches];
    CommonKey k[kCommonSearches];
    for (int g = 0; g < kCommonSearches; ++g) mid[g] = lo[g] < hi[g] ? lo[g] + (hi[g] - lo[g]) / 2 : safe;
    for (int g = 0; g < kCommonSearches; ++g) k[g] = common_key_at(a, mid[g]);
    any = false;
    for (int g = 0; g < kCommonSearches; ++g) {
      if (lo[g] < hi[g]) {
        if (common_key_less(k[g], key)) lo[g] = mid[g] + 1;
        else hi[g] = mid[g];
      }
      any = any || lo[g] < hi[g];
    }
  }
  for (int g = 0; g < kCommonSearches; ++g) {
    const bool inside = lo[g] < end[g];
    const CommonKey k = common_key_at(a, inside ? lo[g] : safe);
    found[g] = inside && common_key_equal(k, key) ? lo[g] : -1;
  }
}

// ---- what a lane of each pass does (i: a site's index in the concatenated arrays; s: its sample)
ABN_HOST_DEVICE inline void common_runs_lane(const CommonSites& a, const long long* site_off, int s, long long i,
                                             long long* run_begin, long long* err) {
  const int32_t c = a.chromosome[i];
  if (!common_key_valid(c, a.strand[i])) {
    common_min(&err[kCommonBadKey], i);
    return;
  }
  if (i == site_off[s] || a.chromosome[i - 1] != c) common_min(&run_begin[(long long)s * kCommonChroms + c], i);
  else if (!common_key_less(common_key_at(a, i - 1), common_key_at(a, i))) common_min(&err[kCommonNotAscending], i);
}

ABN_HOST_DEVICE inline void common_ends_lane(const CommonSites& a, const long long* site_off, int s, long long i,
                                             const long long* run_begin, long long* run_end, long long* err) {
  const int32_t c = a.chromosome[i];
  if (!common_key_valid(c, a.strand[i])) return;
  const long long at = (long long)s * kCommonChroms + c;
  if ((i == site_off[s] || a.chromosome[i - 1] != c) && run_begin[at] != i) common_min(&err[kCommonSplitRun], i);
  if (i + 1 == site_off[s + 1] || a.chromosome[i + 1] != c) run_end[at] = i + 1;
}

// probe site j (of Lp): match [n x Lp] receives where every sample holds its key (the probe: j itself); true: in all
ABN_HOST_DEVICE inline bool common_match_lane(const CommonSites& a, const long long* site_off, int n, int probe,
                                              long long Lp, long long j, const long long* run_begin,
                                              const long long* run_end, uint32_t* match) {
  const long long i = site_off[probe] + j;
  const int32_t c = a.chromosome[i];
  const CommonKey key = common_key_at(a, i);
  match[(long long)probe * Lp + j] = (uint32_t)j;
  if (!common_key_valid(c, key.strand)) return false;
  for (int s0 = 0; s0 < n; s0 += kCommonSearches) {
    int samples[kCommonSearches];
    long long found[kCommonSearches];
    for (int g = 0; g < kCommonSearches; ++g) samples[g] = s0 + g < n && s0 + g != probe ? s0 + g : -1;
    common_find(a, run_begin, run_end, samples, c, key, i, found);
    bool all = true;
    for (int g = 0; g < kCommonSearches; ++g) {
      if (samples[g] < 0) continue;
      if (found[g] < 0) all = false;
      else match[(long long)samples[g] * Lp + j] = (uint32_t)(found[g] - site_off[samples[g]]);
    }
    if (!all) return false;
  }
  return true;
}

// sample s, rank k (of n_common); src [n x Lp]
ABN_HOST_DEVICE inline void common_gather_lane(const CommonSites& a, const long long* site_off, int probe, long long Lp,
                                               long long n_common, int s, long long k, const uint32_t* src, uint8_t* keep,
                                               const CommonGather& g, long long* err) {
  const uint32_t li = src[(long long)s * Lp + k];
  const long long i = site_off[s] + li, ip = site_off[probe] + src[(long long)probe * Lp + k];
  if ((k > 0 && src[(long long)s * Lp + k - 1] >= li) || a.chromosome[i] != a.chromosome[ip] ||
      !common_key_equal(common_key_at(a, i), common_key_at(a, ip)))
    common_min(&err[kCommonNotCoordered], i);
  if (s != probe) keep[i] = 1;  // (the probe's: the match's)
  const long long d = (long long)s * n_common + k;
  if (g.chromosome) g.chromosome[d] = a.chromosome[i];
  if (g.start) g.start[d] = a.start[i];
  if (g.end) g.end[d] = a.end[i];
  if (g.strand) g.strand[d] = a.strand[i];
  if (g.level) g.level[d] = g.level_in[i];
  if (g.code) g.code[(long long)s * g.code_stride + k] = g.code_in[i];
}

// ---- the refusal: which of the order checks failed first, and its text (the host library and the device path share it)
inline CommonRefusal common_refusal(const long long* err, int first, int last, const long long* site_off, int n) {
  CommonRefusal r{0, -1, -1};
  long long at = kCommonNone;
  for (int k = first; k <= last; ++k)
    if (err[k] < at) at = err[k], r.kind = k + 1;
  if (r.kind) {
    r.sample = common_sample_of(site_off, n, at);
    r.site = at - site_off[r.sample];
  }
  return r;
}

inline std::string common_refusal_text(const CommonRefusal& r) {
  const std::string where = "sample " + std::to_string(r.sample) + ", site " + std::to_string(r.site) + ": ";
  switch (r.kind - 1) {
    case kCommonSplitRun: return where + "split run: its chromosome has an earlier run in this sample";
    case kCommonNotAscending: return where + "not ascending: (start, end, strand) is not above the site before it";
    case kCommonBadKey: return where + "a chromosome outside 0..257, or a strand above 2";
    case kCommonNotCoordered: return where + "not co-ordered: the common sites come in another order than in the shortest sample";
  }
  return "";
}

// The whole step, serially, pass by pass as the device runs it.  keep [site_off[n]] is written whenever the order checks
// pass; the return value is n_common, or -1 with *refusal set.
inline long long sites_common_serial(const CommonSites& a, int n, const long long* site_off, uint8_t* keep,
                                     CommonRefusal* refusal) {
  const long long S = site_off[n];
  std::vector<long long> run_begin((size_t)n * kCommonChroms, kCommonNone), run_end((size_t)n * kCommonChroms, 0);
  long long err[kCommonErrs] = {kCommonNone, kCommonNone, kCommonNone, kCommonNone};
  for (long long i = 0; i < S; ++i) keep[i] = 0;
  for (long long i = 0; i < S; ++i)
    common_runs_lane(a, site_off, common_sample_of(site_off, n, i), i, run_begin.data(), err);
  for (long long i = 0; i < S; ++i)
    common_ends_lane(a, site_off, common_sample_of(site_off, n, i), i, run_begin.data(), run_end.data(), err);
  *refusal = common_refusal(err, kCommonSplitRun, kCommonBadKey, site_off, n);
  if (refusal->kind) return -1;
  const int probe = common_pick_probe(site_off, n);
  const long long Lp = site_off[probe + 1] - site_off[probe];
  std::vector<uint32_t> match((size_t)n * (size_t)Lp), src((size_t)n * (size_t)Lp);
  long long n_common = 0;
  for (long long j = 0; j < Lp; ++j)
    if (common_match_lane(a, site_off, n, probe, Lp, j, run_begin.data(), run_end.data(), match.data())) {
      keep[site_off[probe] + j] = 1;
      for (int s = 0; s < n; ++s) src[(size_t)s * (size_t)Lp + (size_t)n_common] = match[(size_t)s * (size_t)Lp + (size_t)j];
      ++n_common;
    }
  const CommonGather none{};
  for (int s = 0; s < n; ++s)
    for (long long k = 0; k < n_common; ++k)
      common_gather_lane(a, site_off, probe, Lp, n_common, s, k, src.data(), keep, none, err);
  *refusal = common_refusal(err, kCommonNotCoordered, kCommonNotCoordered, site_off, n);
  return refusal->kind ? -1 : n_common;
}

#if defined(__HIPCC__) && (defined(ABN_SITES_COMMON_KERNELS) || defined(ABN_SITES_UNION_KERNELS))
// The exclusive rank of `flag` among the workgroup's lanes, and their number: ballots inside a wavefront, the four
// wavefronts' counts through LDS.  Every lane of the workgroup calls it.  (Shared with abn_sites_union.hpp's kernels.)
__device__ inline uint32_t common_block_rank(bool flag, uint32_t* s_wave, uint32_t& total) {
  const unsigned long long mask = __ballot(flag);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) s_wave[wave] = (uint32_t)__popcll(mask);
  __syncthreads();
  uint32_t before = 0;
  total = 0;
  for (int w = 0; w < kCommonThreads / 64; ++w) {
    if (w < wave) before += s_wave[w];
    total += s_wave[w];
  }
  return before + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
}
#endif

#if defined(__HIPCC__) && defined(ABN_SITES_COMMON_KERNELS)  // (abn_sites_common.hip defines it)
// ------------------------------------------------------------------------------------------------ kernels
// grid: ceil(S / kCommonThreads), S = site_off[n] sites
__global__ void __launch_bounds__(kCommonThreads)
abn_common_runs_kernel(CommonSites a, const long long* __restrict__ site_off, int n, long long* __restrict__ run_begin,
                       long long* __restrict__ err) {
  const long long i = (long long)blockIdx.x * kCommonThreads + threadIdx.x;
  if (i < site_off[n]) common_runs_lane(a, site_off, common_sample_of(site_off, n, i), i, run_begin, err);
}

__global__ void __launch_bounds__(kCommonThreads)
abn_common_ends_kernel(CommonSites a, const long long* __restrict__ site_off, int n, const long long* __restrict__ run_begin,
                       long long* __restrict__ run_end, long long* __restrict__ err) {
  const long long i = (long long)blockIdx.x * kCommonThreads + threadIdx.x;
  if (i < site_off[n]) common_ends_lane(a, site_off, common_sample_of(site_off, n, i), i, run_begin, run_end, err);
}

// grid: ceil(Lp / kCommonThreads); keep: the probe's flags, at its first site
__global__ void __launch_bounds__(kCommonThreads)
abn_common_match_kernel(CommonSites a, const long long* __restrict__ site_off, int n, int probe, long long Lp,
                        const long long* __restrict__ run_begin, const long long* __restrict__ run_end,
                        uint32_t* __restrict__ match, uint8_t* __restrict__ keep, uint32_t* __restrict__ block_count) {
  __shared__ uint32_t s_wave[kCommonThreads / 64];
  const long long j = (long long)blockIdx.x * kCommonThreads + threadIdx.x;
  bool kept = false;
  if (j < Lp) {
    kept = common_match_lane(a, site_off, n, probe, Lp, j, run_begin, run_end, match);
    keep[j] = kept ? 1 : 0;
  }
  uint32_t total;
  (void)common_block_rank(kept, s_wave, total);
  if (threadIdx.x == 0) block_count[blockIdx.x] = total;
}

// one workgroup: data[0 .. n) scanned in place (exclusive), the sum at data[n]
__global__ void __launch_bounds__(kCommonThreads)
abn_common_scan_kernel(uint32_t* __restrict__ data, uint32_t n) {
  __shared__ uint32_t s_part[kCommonThreads];
  const uint32_t per = (n + kCommonThreads - 1) / kCommonThreads;
  const uint32_t lo = min(threadIdx.x * per, n), hi = min(lo + per, n);
  uint32_t sum = 0;
  for (uint32_t i = lo; i < hi; ++i) sum += data[i];
  s_part[threadIdx.x] = sum;
  __syncthreads();
  for (int d = 1; d < kCommonThreads; d <<= 1) {  // Hillis-Steele, inclusive
    const uint32_t up = threadIdx.x >= (unsigned)d ? s_part[threadIdx.x - d] : 0u;
    __syncthreads();
    s_part[threadIdx.x] += up;
    __syncthreads();
  }
  uint32_t run = s_part[threadIdx.x] - sum;
  for (uint32_t i = lo; i < hi; ++i) {
    const uint32_t c = data[i];
    data[i] = run;
    run += c;
  }
  if (threadIdx.x == kCommonThreads - 1) data[n] = s_part[threadIdx.x];
}

// grid: (ceil(Lp / kCommonThreads), n); keep: the probe's flags; block_off: the scanned counts
__global__ void __launch_bounds__(kCommonThreads)
abn_common_rank_kernel(const uint8_t* __restrict__ keep, long long Lp, const uint32_t* __restrict__ block_off,
                       const uint32_t* __restrict__ match, uint32_t* __restrict__ src) {
  __shared__ uint32_t s_wave[kCommonThreads / 64];
  const long long j = (long long)blockIdx.x * kCommonThreads + threadIdx.x;
  const bool kept = j < Lp && keep[j] != 0;
  uint32_t total;
  const uint32_t k = block_off[blockIdx.x] + common_block_rank(kept, s_wave, total);
  if (kept) src[(long long)blockIdx.y * Lp + k] = match[(long long)blockIdx.y * Lp + j];
}

// grid: (ceil(n_common / kCommonThreads), n); keep: all samples' flags
__global__ void __launch_bounds__(kCommonThreads)
abn_common_gather_kernel(CommonSites a, const long long* __restrict__ site_off, int probe, long long Lp, long long n_common,
                         const uint32_t* __restrict__ src, uint8_t* __restrict__ keep, CommonGather g,
                         long long* __restrict__ err) {
  const long long k = (long long)blockIdx.x * kCommonThreads + threadIdx.x;
  if (k < n_common) common_gather_lane(a, site_off, probe, Lp, n_common, (int)blockIdx.y, k, src, keep, g, err);
}
#endif  // kernels

}  // namespace abn
