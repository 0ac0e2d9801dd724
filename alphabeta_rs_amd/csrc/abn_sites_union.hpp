// The union of the samples' sites, by genomic position, on the device (abn_sites_union, abn_windows_create_union,
// abn_codes_create_union).  abn_sites_common.hpp reduces the samples to the sites EVERY sample holds; with many samples
// that each lack a few sites little is left, while any two of them still share nearly all.  The comparison the model needs
// is per pair: DMatrix::from (src/pedigree.rs:240-254) skips a site for a pair when either side is filtered and divides by
// the pair's own compared sites.  So this step gives every sample ALL the sites any sample holds — an n-way union join —
// and fills what a sample lacks with a PLACEHOLDER: the union site's key, code 0x80 (status U, filtered), level +0.0.
// The scan, the plans and the fits are untouched; "filtered" is the code they already have for "nothing to say here".
//
// KEY and WELL ORDERED are abn_sites_common.hpp's, and so are its runs / ends passes, their tables and their refusals.
//
// THE UNION ORDER.  Inside a chromosome the distinct keys ascend by common_key_less.  The chromosomes come in the run
// order of the REFERENCE SAMPLE (the one with the most runs, the lowest index among equals); chromosomes it lacks are
// appended in the order they are first met going through the samples 0 .. n-1, each in its run order.  Every sample's run
// order must be a subsequence of that order: a run whose chromosome stands in the union order before the chromosome of
// the sample's run in front of it is OUT OF ORDER and the input is refused (kUnionRunOrder) with the run's first site.
// The order is host arithmetic on the run_begin tables (union_chromosome_order), not a device pass.
//
// The samples' arrays lie one behind the other, S = site_off[n] sites, S below 2^32 (so a site's index, and n_union, fit a
// uint32_t).  An OWNER is the site of the lowest sample that holds a key: every distinct key has exactly one.
//
//   owner   a lane per site i of sample s: its key looked up in the samples t < s, kCommonSearches at a time through
//           common_find, lowest t first, stopping at the first group with a hit.  owner[i] = the hit of the lowest t, or i.
//   scan    P[i] = the number of owners in front of site i (S + 1 entries; P[S] = n_union): the workgroups' owner counts
//           (written by the owner pass), their exclusive scan by abn_common_scan_kernel, and a lane per site adding its
//           rank inside the workgroup.  Two levels, no workgroup waits for another.  The host reads n_union, the error
//           cells and run_begin here.
//   base    count[q] = the distinct keys of the q-th chromosome c of the union order = the sum over the samples t of
//           P[run_end[t][c]] - P[run_begin[t][c]] (a workgroup per q); base[c] = the sum of the counts in front of q.
//   rank    THE HOT PASS.  A lane per owner with key k in chromosome c: r = base[c] + the sum over ALL samples t of
//           P[lb_t(k)] - P[run_begin[t][c]], lb_t the lower bound of k inside sample t's run of c — the owners below k.
//           kCommonSearches samples per step (union_bounds), so as many independent loads are in flight.  A sample
//           without the chromosome contributes 0 and its table entries are not used as indices.
//   dest    a lane per site: dest[i] = r[owner[i]], the site's union rank.
//   invert  a lane per site: inv[s][dest[i]] = i - site_off[s] (inv is filled with kUnionNone in front of the kernel), and
//           the owner writes own_at[dest[i]] = i.  One writer per element: a sample holds a key once, a key has one owner.
//   gather  a lane per (sample, rank): the sample's own site's chromosome, start, end, strand, code and level, or the
//           placeholder with the key of own_at[u].
//
// Plain stores, one writer per output element; the atomicMin of the run tables and the error cells (abn_sites_common.hpp)
// stays the only atomic.  A sample that is not well ordered still gives in-bounds tables, so owner and scan may run before
// the host looks at the error cells; nothing behind the host read runs on a refused input.
//
// Temporaries, from the context's pool: owner, P, r and dest 4 bytes per site each, the two tables of 258 x 8 bytes per
// sample, a count per workgroup, and behind the host read inv (4 bytes x n x n_union) and own_at (4 bytes x n_union).
//
// The lane functions, the order and the whole step in its serial form compile without a HIP header: the host library
// (host_capi.cpp) and tests/native/union_main.cpp include this file as it is.
#pragma once
#include "abn_sites_common.hpp"

namespace abn {

constexpr uint32_t kUnionNone = 0xffffffffu;  // in inv: the sample has no site at this rank (what a byte fill of 0xff leaves)
constexpr uint8_t kUnionPlaceholderCode = 0x80;  // status U, filtered; as a merged byte of abn_codes.hpp: not counted
constexpr int kUnionRunOrder = 5;  // a refusal's kind, behind abn_sites_common.hpp's four (1 + its err entries)
enum { kAlignNone = 0, kAlignPosition = 1, kAlignUnion = 2 };  // how a handle's samples are aligned in front of its build
constexpr int kUnionPasses = 8;    // runs and ends, owner, scan, base, rank, dest, invert, gather

// the lower bounds of `key` inside the runs of chromosome `chromosome` (valid) of kCommonSearches samples at once:
// lb[g] in [begin[g], end[g]] and begin[g] = the run's begin, or has[g] = false (no sample, or it lacks the chromosome) and
// both 0.  The loads of a step are independent of one another; a search that is over reads the site `safe` and ignores it.
ABN_HOST_DEVICE inline void union_bounds(const CommonSites& a, const long long* run_begin, const long long* run_end,
                                         const int samples[kCommonSearches], int chromosome, const CommonKey& key,
                                         long long safe, long long begin[kCommonSearches], long long lb[kCommonSearches],
                                         bool has[kCommonSearches]) {
  long long lo[kCommonSearches], hi[kCommonSearches];
  bool any = false;
  for (int g = 0; g < kCommonSearches; ++g) {
    lo[g] = hi[g] = begin[g] = 0;
    has[g] = false;
    if (samples[g] >= 0) {
      const long long at = (long long)samples[g] * kCommonChroms + chromosome;
      const long long b = run_begin[at], e = run_end[at];  // (a chromosome the sample lacks: begin kCommonNone, end 0)
      if (b < e) lo[g] = begin[g] = b, hi[g] = e, has[g] = true;
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
  for (int g = 0; g < kCommonSearches; ++g) lb[g] = lo[g];
}

// ---- what a lane of each pass does (i: a site's index in the concatenated arrays; s: its sample)
// returns whether site i is an owner
ABN_HOST_DEVICE inline bool union_owner_lane(const CommonSites& a, int s, long long i, const long long* run_begin,
                                             const long long* run_end, uint32_t* owner) {
  const int32_t c = a.chromosome[i];
  const CommonKey key = common_key_at(a, i);
  long long at = i;
  if (common_key_valid(c, key.strand))  // (else: refused behind the scan; no index into the tables)
    for (int t0 = 0; t0 < s && at == i; t0 += kCommonSearches) {
      int samples[kCommonSearches];
      long long found[kCommonSearches];
      for (int g = 0; g < kCommonSearches; ++g) samples[g] = t0 + g < s ? t0 + g : -1;
      common_find(a, run_begin, run_end, samples, c, key, i, found);
      for (int g = kCommonSearches - 1; g >= 0; --g)
        if (found[g] >= 0) at = found[g];  // (the lowest sample of the group stays)
    }
  owner[i] = (uint32_t)at;
  return at == i;
}

// the distinct keys sample t brings to chromosome c: the owners inside its run
ABN_HOST_DEVICE inline uint32_t union_count_lane(const uint32_t* P, const long long* run_begin, const long long* run_end,
                                                 int t, int c) {
  const long long at = (long long)t * kCommonChroms + c;
  const long long b = run_begin[at], e = run_end[at];
  return b < e ? P[e] - P[b] : 0u;
}

// owner site i (owner[i] == i): its union rank
ABN_HOST_DEVICE inline uint32_t union_rank_lane(const CommonSites& a, int n, long long i, const long long* run_begin,
                                                const long long* run_end, const uint32_t* P, const uint32_t* base) {
  const int32_t c = a.chromosome[i];
  const CommonKey key = common_key_at(a, i);
  uint32_t r = base[c];
  for (int t0 = 0; t0 < n; t0 += kCommonSearches) {
    int samples[kCommonSearches];
    long long begin[kCommonSearches], lb[kCommonSearches];
    bool has[kCommonSearches];
    for (int g = 0; g < kCommonSearches; ++g) samples[g] = t0 + g < n ? t0 + g : -1;
    union_bounds(a, run_begin, run_end, samples, c, key, i, begin, lb, has);
    uint32_t above[kCommonSearches], below[kCommonSearches];
    for (int g = 0; g < kCommonSearches; ++g) above[g] = P[has[g] ? lb[g] : 0], below[g] = P[has[g] ? begin[g] : 0];
    for (int g = 0; g < kCommonSearches; ++g) r += has[g] ? above[g] - below[g] : 0u;
  }
  return r;
}

ABN_HOST_DEVICE inline void union_dest_lane(long long i, const uint32_t* owner, const uint32_t* r, uint32_t* dest) {
  dest[i] = r[owner[i]];
}

// inv [n x n_union], own_at [n_union]
ABN_HOST_DEVICE inline void union_invert_lane(const long long* site_off, int s, long long i, long long n_union,
                                              const uint32_t* owner, const uint32_t* dest, uint32_t* inv, uint32_t* own_at) {
  inv[(long long)s * n_union + dest[i]] = (uint32_t)(i - site_off[s]);
  if (owner[i] == (uint32_t)i) own_at[dest[i]] = (uint32_t)i;
}

// sample s, union rank u; g as abn_sites_common.hpp's gather, with n_union for its n_common
ABN_HOST_DEVICE inline void union_gather_lane(const CommonSites& a, const long long* site_off, long long n_union, int s,
                                              long long u, const uint32_t* inv, const uint32_t* own_at,
                                              const CommonGather& g) {
  const uint32_t li = inv[(long long)s * n_union + u];
  const bool mine = li != kUnionNone;
  const long long i = mine ? site_off[s] + li : (long long)own_at[u];  // the key's site: the sample's own, or the owner's
  const long long d = (long long)s * n_union + u;
  if (g.chromosome) g.chromosome[d] = a.chromosome[i];
  if (g.start) g.start[d] = a.start[i];
  if (g.end) g.end[d] = a.end[i];
  if (g.strand) g.strand[d] = a.strand[i];
  if (g.level) g.level[d] = mine ? g.level_in[i] : 0.0;
  if (g.code) g.code[(long long)s * g.code_stride + u] = mine ? g.code_in[i] : kUnionPlaceholderCode;
}

// ---- the union order of the chromosomes, from the run_begin table [n x 258] of well ordered samples
// order: the chromosomes in union order.  Returns the lowest first site of an out-of-order run, or kCommonNone.
inline long long union_chromosome_order(const long long* run_begin, int n, std::vector<int>& order) {
  std::vector<std::vector<int>> runs((size_t)n);  // every sample's chromosomes in run order
  int ref = 0;
  for (int s = 0; s < n; ++s) {
    const long long* b = run_begin + (size_t)s * kCommonChroms;
    std::vector<int>& mine = runs[(size_t)s];
    for (int c = 0; c < kCommonChroms; ++c)
      if (b[c] != kCommonNone) mine.push_back(c);
    for (size_t k = 1; k < mine.size(); ++k)  // insertion sort by begin: few runs
      for (size_t j = k; j > 0 && b[mine[j]] < b[mine[j - 1]]; --j) {
        const int x = mine[j];
        mine[j] = mine[j - 1], mine[j - 1] = x;
      }
    if (mine.size() > runs[(size_t)ref].size()) ref = s;
  }
  int pos[kCommonChroms];
  for (int c = 0; c < kCommonChroms; ++c) pos[c] = -1;
  order.clear();
  auto take = [&](const std::vector<int>& mine) {
    for (int c : mine)
      if (pos[c] < 0) pos[c] = (int)order.size(), order.push_back(c);
  };
  if (n > 0) take(runs[(size_t)ref]);
  for (int s = 0; s < n; ++s) take(runs[(size_t)s]);
  long long at = kCommonNone;
  for (int s = 0; s < n && at == kCommonNone; ++s) {  // (begins ascend with the sample: the first sample's is the lowest)
    const std::vector<int>& mine = runs[(size_t)s];
    for (size_t k = 1; k < mine.size(); ++k)
      if (pos[mine[k]] < pos[mine[k - 1]]) {
        at = run_begin[(size_t)s * kCommonChroms + (size_t)mine[k]];
        break;
      }
  }
  return at;
}

inline std::string union_refusal_text(const CommonRefusal& r) {
  if (r.kind == kUnionRunOrder)
    return "sample " + std::to_string(r.sample) + ", site " + std::to_string(r.site) +
           ": run order: this run's chromosome comes before the chromosome of the run in front of it in the union order";
  return common_refusal_text(r);
}

// the run-order refusal from the host's tables, and the order
inline CommonRefusal union_order_refusal(const long long* run_begin, const long long* site_off, int n, std::vector<int>& order) {
  CommonRefusal r{0, -1, -1};
  const long long at = union_chromosome_order(run_begin, n, order);
  if (at != kCommonNone) {
    r.kind = kUnionRunOrder;
    r.sample = common_sample_of(site_off, n, at);
    r.site = at - site_off[r.sample];
  }
  return r;
}

// The whole step, serially, pass by pass as the device runs it.  dest [site_off[n]] is written whenever the input is not
// refused; g's outputs (any may be null; n_union sites per sample) are filled when fill is given: it is called with n_union
// before the gather so that the caller can size them.  The return value is n_union, or -1 with *refusal set.
template <class Fill>
inline long long sites_union_serial(const CommonSites& a, int n, const long long* site_off, uint32_t* dest,
                                    CommonRefusal* refusal, Fill fill) {
  const long long S = site_off[n];
  *refusal = CommonRefusal{0, -1, -1};
  if (S > 0xffffffffLL) return -1;
  std::vector<long long> run_begin((size_t)n * kCommonChroms, kCommonNone), run_end((size_t)n * kCommonChroms, 0);
  long long err[kCommonErrs] = {kCommonNone, kCommonNone, kCommonNone, kCommonNone};
  for (long long i = 0; i < S; ++i)
    common_runs_lane(a, site_off, common_sample_of(site_off, n, i), i, run_begin.data(), err);
  for (long long i = 0; i < S; ++i)
    common_ends_lane(a, site_off, common_sample_of(site_off, n, i), i, run_begin.data(), run_end.data(), err);
  std::vector<uint32_t> owner((size_t)S), P((size_t)S + 1), r((size_t)S, 0);
  uint32_t owners = 0;
  for (long long i = 0; i < S; ++i) {
    P[(size_t)i] = owners;
    owners += union_owner_lane(a, common_sample_of(site_off, n, i), i, run_begin.data(), run_end.data(), owner.data()) ? 1u : 0u;
  }
  P[(size_t)S] = owners;
  *refusal = common_refusal(err, kCommonSplitRun, kCommonBadKey, site_off, n);
  if (refusal->kind) return -1;
  std::vector<int> order;
  *refusal = union_order_refusal(run_begin.data(), site_off, n, order);
  if (refusal->kind) return -1;
  const long long n_union = owners;
  uint32_t base[kCommonChroms] = {0};
  uint32_t before = 0;
  for (int c : order) {
    base[c] = before;
    for (int t = 0; t < n; ++t) before += union_count_lane(P.data(), run_begin.data(), run_end.data(), t, c);
  }
  for (long long i = 0; i < S; ++i)
    if (owner[(size_t)i] == (uint32_t)i)
      r[(size_t)i] = union_rank_lane(a, n, i, run_begin.data(), run_end.data(), P.data(), base);
  for (long long i = 0; i < S; ++i) union_dest_lane(i, owner.data(), r.data(), dest);
  std::vector<uint32_t> inv((size_t)n * (size_t)n_union, kUnionNone), own_at((size_t)n_union);
  for (long long i = 0; i < S; ++i)
    union_invert_lane(site_off, common_sample_of(site_off, n, i), i, n_union, owner.data(), dest, inv.data(), own_at.data());
  const CommonGather g = fill(n_union);
  for (int s = 0; s < n; ++s)
    for (long long u = 0; u < n_union; ++u) union_gather_lane(a, site_off, n_union, s, u, inv.data(), own_at.data(), g);
  return n_union;
}

inline long long sites_union_serial(const CommonSites& a, int n, const long long* site_off, uint32_t* dest,
                                    CommonRefusal* refusal) {
  return sites_union_serial(a, n, site_off, dest, refusal, [](long long) { return CommonGather{}; });
}

#if defined(__HIPCC__) && defined(ABN_SITES_UNION_KERNELS)  // (abn_sites_union.hip defines it)
// ------------------------------------------------------------------------------------------------ kernels
// grid: ceil(S / kCommonThreads); block_count: every workgroup's owners
__global__ void __launch_bounds__(kCommonThreads)
abn_union_owner_kernel(CommonSites a, const long long* __restrict__ site_off, int n, const long long* __restrict__ run_begin,
                       const long long* __restrict__ run_end, uint32_t* __restrict__ owner,
                       uint32_t* __restrict__ block_count) {
  __shared__ uint32_t s_wave[kCommonThreads / 64];
  const long long i = (long long)blockIdx.x * kCommonThreads + threadIdx.x;
  bool own = false;
  if (i < site_off[n]) own = union_owner_lane(a, common_sample_of(site_off, n, i), i, run_begin, run_end, owner);
  uint32_t total;
  (void)common_block_rank(own, s_wave, total);
  if (threadIdx.x == 0) block_count[blockIdx.x] = total;
}

// grid: ceil(S / kCommonThreads); block_off: the scanned counts, the sum behind them (n_blocks entries + 1)
__global__ void __launch_bounds__(kCommonThreads)
abn_union_prefix_kernel(long long S, const uint32_t* __restrict__ owner, const uint32_t* __restrict__ block_off,
                        uint32_t n_blocks, uint32_t* __restrict__ P) {
  __shared__ uint32_t s_wave[kCommonThreads / 64];
  const long long i = (long long)blockIdx.x * kCommonThreads + threadIdx.x;
  const bool own = i < S && owner[i] == (uint32_t)i;
  uint32_t total;
  const uint32_t before = block_off[blockIdx.x] + common_block_rank(own, s_wave, total);
  if (i < S) P[i] = before;
  if (i == S - 1) P[S] = block_off[n_blocks];
}

// grid: the chromosomes of the union order, a workgroup each; count [n_order]
__global__ void __launch_bounds__(kCommonThreads)
abn_union_count_kernel(const uint32_t* __restrict__ P, const long long* __restrict__ run_begin,
                       const long long* __restrict__ run_end, int n, const int* __restrict__ order,
                       uint32_t* __restrict__ count) {
  __shared__ uint32_t s_part[kCommonThreads];
  const int c = order[blockIdx.x];
  uint32_t sum = 0;
  for (int t = threadIdx.x; t < n; t += kCommonThreads) sum += union_count_lane(P, run_begin, run_end, t, c);
  s_part[threadIdx.x] = sum;
  __syncthreads();
  for (int d = kCommonThreads / 2; d > 0; d >>= 1) {
    if (threadIdx.x < (unsigned)d) s_part[threadIdx.x] += s_part[threadIdx.x + d];
    __syncthreads();
  }
  if (threadIdx.x == 0) count[blockIdx.x] = s_part[0];
}

// one lane: base [258] from the counts, in union order (at most 258 additions)
__global__ void abn_union_base_kernel(const uint32_t* __restrict__ count, const int* __restrict__ order, int n_order,
                                      uint32_t* __restrict__ base) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  uint32_t before = 0;
  for (int q = 0; q < n_order; ++q) {
    base[order[q]] = before;
    before += count[q];
  }
}

// grid: ceil(S / kCommonThreads)
__global__ void __launch_bounds__(kCommonThreads)
abn_union_rank_kernel(CommonSites a, long long S, int n, const long long* __restrict__ run_begin,
                      const long long* __restrict__ run_end, const uint32_t* __restrict__ owner,
                      const uint32_t* __restrict__ P, const uint32_t* __restrict__ base, uint32_t* __restrict__ r) {
  const long long i = (long long)blockIdx.x * kCommonThreads + threadIdx.x;
  if (i < S && owner[i] == (uint32_t)i) r[i] = union_rank_lane(a, n, i, run_begin, run_end, P, base);
}

__global__ void __launch_bounds__(kCommonThreads)
abn_union_dest_kernel(long long S, const uint32_t* __restrict__ owner, const uint32_t* __restrict__ r,
                      uint32_t* __restrict__ dest) {
  const long long i = (long long)blockIdx.x * kCommonThreads + threadIdx.x;
  if (i < S) union_dest_lane(i, owner, r, dest);
}

__global__ void __launch_bounds__(kCommonThreads)
abn_union_invert_kernel(const long long* __restrict__ site_off, int n, long long n_union, const uint32_t* __restrict__ owner,
                        const uint32_t* __restrict__ dest, uint32_t* __restrict__ inv, uint32_t* __restrict__ own_at) {
  const long long i = (long long)blockIdx.x * kCommonThreads + threadIdx.x;
  if (i < site_off[n]) union_invert_lane(site_off, common_sample_of(site_off, n, i), i, n_union, owner, dest, inv, own_at);
}

// grid: (ceil(n_union / kCommonThreads), n)
__global__ void __launch_bounds__(kCommonThreads)
abn_union_gather_kernel(CommonSites a, const long long* __restrict__ site_off, long long n_union,
                        const uint32_t* __restrict__ inv, const uint32_t* __restrict__ own_at, CommonGather g) {
  const long long u = (long long)blockIdx.x * kCommonThreads + threadIdx.x;
  if (u < n_union) union_gather_lane(a, site_off, n_union, (int)blockIdx.y, u, inv, own_at, g);
}
#endif  // kernels

}  // namespace abn
