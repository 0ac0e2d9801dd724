// Repeated sites of one resident methylome collapsed on the device (abn_sites_dedup, abn_sites_dedup_keys): of every RUN —
// a maximal stretch of consecutive records with equal keys (chromosome, start, end, strand; sort_key_compare of
// abn_sites_sort.hpp) — at most one record is kept, by a policy, and the kept records keep their order.  The input has no
// descent in canonical order: it is what abn_sites_sort leaves, whose stable sort keeps repeated keys adjacent and in file
// order.
//
//   FIRST, LAST  the first, the last record of the run in input order
//   BEST         the record with the highest posteriormax: dedup_better walks the run from its first record, so a tie —
//                -0.0 and +0.0 tie — keeps the earlier record, a NaN loses against every number, and a run of only NaN
//                keeps its first record
//   DROP         no record of a run longer than one
// A run of one record is always kept.
//
//   abn_sort_flatten_*_kernel  (abn_sites_sort.hpp, as they are) the sample's records in file order with the whole record
//   abn_dedup_flags_kernel     a lane per record, at most kSortCheckBlocks workgroups striding: its key against its
//                              predecessor's and its successor's, both read from global memory, so no wavefront, workgroup
//                              or stride boundary is special.  head = no equal predecessor, tail = no equal successor;
//                              keep[i] = head (FIRST), tail (LAST), head and tail (DROP).  Per workgroup one partial record
//                              comes to the host: the first descent's index (min), the keys outside their ranges, the heads
//                              that are no tails (the repeated keys), the neighbours of equal key whose status differs.
//                              BEST: the lane of a head that is a tail writes keep[i] = 1; the lane of a head that is no
//                              tail WALKS its run in global memory with dedup_better and then writes keep of every record
//                              of the run; the other lanes write nothing.  So every keep byte has one writer: a record's own
//                              lane, or — BEST, in a run of several — the lane of the run's head.
//   abn_dedup_count_kernel     a workgroup per tile of kSortTile records: count[tile] = its keep flags, a ballot and a
//                              popcount per wavefront and item
//   abn_parse_scan_kernel      (abn_parse_kernels.hpp) one workgroup: the exclusive scan of the tile counts, the number of
//                              kept records behind them
//   abn_dedup_scatter_kernel   a workgroup per tile: order[rank] = index for every kept record, rank = (kept in earlier
//                              tiles: the scan) + (kept in earlier groups of 64 of the tile: LDS) + (kept in front of it in
//                              its group: the ballot's popcount below the lane) — ascending along the input
//   abn_dedup_gather_kernel    a lane per output record: the record arrays copied from order[k], line = k
//
// Nothing comes from an atomic's return value (there is no atomic), every output element has one writer and a plain vector
// store, no workgroup waits for another, and no kernel uses scratch.
//
// What BEST costs: the walk is SERIAL in the run's length — one lane reads the run's keys and posteriors one after the
// other, twice the keys (the walk, then the write of the flags).  A run is as long as the number of replicates of a site,
// a handful in practice, and the runs are walked side by side.  The pathological file, every key equal, is one run: one
// lane walks all n records while every other lane idles — n dependent global reads, about a microsecond each, so seconds
// for millions of records where the other policies take microseconds.  The result is still right; nothing bounds the run.
//
// The flags, the walk and the compaction in their serial forms compile without a HIP header: the host library
// (host_capi.cpp) and tests/native/sites_dedup_main.cpp include this file as it is.
#pragma once
#include <stdint.h>

#include <vector>

#include "abn_sites_sort.hpp"

namespace abn {

constexpr int kDedupFirst = 0, kDedupLast = 1, kDedupBest = 2, kDedupDrop = 3;  // ABN_DEDUP_* of include/abneutral.h
constexpr int kDedupPartialWords = 4;  // first descent (min; kDedupNoDescent: none), bad keys, repeated keys, disagreeing
constexpr uint32_t kDedupNoDescent = 0xffffffffu;

ABN_HOST_DEVICE inline bool dedup_policy_valid(int policy) { return policy >= kDedupFirst && policy <= kDedupDrop; }

// BEST's comparison, walking a run in input order from its first record: does `candidate` replace `best`?
ABN_HOST_DEVICE inline bool dedup_better(double candidate, double best) {
  return candidate > best || (best != best && candidate == candidate);
}

// Where the kernels and the serial forms read a record's key, posterior and status: the six arrays of the primitive, or a
// flattened sample's meta, start, end and posteriormax
struct DedupArrays {
  const int32_t* chromosome;
  const uint32_t* start;
  const uint32_t* end;
  const uint8_t* strand;
  const double* posteriormax;
  const uint8_t* status_;
  ABN_HOST_DEVICE SortKey key(long long i) const { return sort_key((uint32_t)chromosome[i], start[i], end[i], strand[i]); }
  ABN_HOST_DEVICE bool valid(long long i) const { return sort_key_valid(chromosome[i], strand[i]); }
  ABN_HOST_DEVICE double posterior(long long i) const { return posteriormax[i]; }
  ABN_HOST_DEVICE uint32_t status(long long i) const { return status_[i]; }
};
struct DedupMeta {
  const uint32_t* meta;
  const uint32_t* start;
  const uint32_t* end;
  const double* posteriormax;
  ABN_HOST_DEVICE SortKey key(long long i) const { return sort_key_of_meta(meta[i], start[i], end[i]); }
  ABN_HOST_DEVICE bool valid(long long i) const { return sort_key_valid(meta_chromosome(meta[i]), meta_strand(meta[i])); }
  ABN_HOST_DEVICE double posterior(long long i) const { return posteriormax[i]; }
  ABN_HOST_DEVICE uint32_t status(long long i) const { return meta_status(meta[i]); }
};

// What the flags pass finds, added up (the descent: the minimum) over its lanes
struct DedupCheck {
  uint32_t descent = kDedupNoDescent;  // the first record whose key lies below its predecessor's
  uint32_t bad = 0, repeated = 0, disagreeing = 0;
  ABN_HOST_DEVICE void add(const DedupCheck& o) {
    descent = o.descent < descent ? o.descent : descent;
    bad += o.bad, repeated += o.repeated, disagreeing += o.disagreeing;
  }
};

// BEST, the lane of a head that is no tail: the walk of the run that begins at record i (key k) and the keep flags of all
// its records.  Reads and writes stay below n
template <class Keys>
ABN_HOST_DEVICE inline void dedup_walk_run(const Keys& keys, long long i, long long n, const SortKey& k, uint8_t* keep) {
  long long best = i, j = i + 1;
  double best_pm = keys.posterior(i);
  for (; j < n; ++j) {
    const SortKey q = keys.key(j);
    if (sort_key_compare(q.w, k.w) != 0) break;
    const double pm = keys.posterior(j);
    if (dedup_better(pm, best_pm)) best = j, best_pm = pm;
  }
  for (long long r = i; r < j; ++r) keep[r] = r == best ? 1 : 0;
}

// One record's flags: what a lane of abn_dedup_flags_kernel does with record i of n
template <class Keys>
ABN_HOST_DEVICE inline void dedup_flags_record(const Keys& keys, long long i, long long n, int policy, uint8_t* keep,
                                               DedupCheck& check) {
  const SortKey k = keys.key(i);
  check.bad += keys.valid(i) ? 0u : 1u;
  bool head = true, tail = true;
  if (i > 0) {
    const SortKey p = keys.key(i - 1);
    const int cmp = sort_key_compare(k.w, p.w);
    head = cmp != 0;
    if (cmp < 0 && (uint32_t)i < check.descent) check.descent = (uint32_t)i;
    if (cmp == 0 && keys.status(i) != keys.status(i - 1)) ++check.disagreeing;
  }
  if (i + 1 < n) {
    const SortKey s = keys.key(i + 1);
    tail = sort_key_compare(s.w, k.w) != 0;
  }
  if (head && !tail) ++check.repeated;
  switch (policy) {
    case kDedupFirst: keep[i] = head ? 1 : 0; break;
    case kDedupLast: keep[i] = tail ? 1 : 0; break;
    case kDedupDrop: keep[i] = head && tail ? 1 : 0; break;
    default:  // BEST
      if (head && tail) keep[i] = 1;
      else if (head) dedup_walk_run(keys, i, n, k, keep);
      break;
  }
}

// ---- serial forms
// The reference form: run after run.  order has room for n entries and receives the kept records' indices, ascending;
// info4 = {n, kept, repeated keys, disagreeing neighbours}.  0, or 1: a key outside its ranges (*first_descent = -1) or a
// descent (*first_descent = the first record whose key lies below its predecessor's); nothing else is written then
template <class Keys>
inline int dedup_serial(const Keys& keys, long long n, int policy, long long* order, long long* info4,
                        long long* first_descent) {
  *first_descent = -1;
  for (long long i = 0; i < n; ++i)
    if (!keys.valid(i)) return 1;
  for (long long i = 1; i < n; ++i) {
    const SortKey a = keys.key(i), b = keys.key(i - 1);
    if (sort_key_compare(a.w, b.w) < 0) {
      *first_descent = i;
      return 1;
    }
  }
  long long kept = 0, repeated = 0, disagreeing = 0;
  for (long long lo = 0; lo < n;) {
    const SortKey k = keys.key(lo);
    long long hi = lo + 1;
    for (; hi < n; ++hi) {
      const SortKey q = keys.key(hi);
      if (sort_key_compare(q.w, k.w) != 0) break;
      disagreeing += keys.status(hi) != keys.status(hi - 1);
    }
    if (hi - lo == 1) {
      order[kept++] = lo;
    } else {
      ++repeated;
      if (policy == kDedupFirst) order[kept++] = lo;
      else if (policy == kDedupLast) order[kept++] = hi - 1;
      else if (policy == kDedupBest) {
        long long best = lo;
        for (long long j = lo + 1; j < hi; ++j)
          if (dedup_better(keys.posterior(j), keys.posterior(best))) best = j;
        order[kept++] = best;
      }
    }
    lo = hi;
  }
  info4[0] = n, info4[1] = kept, info4[2] = repeated, info4[3] = disagreeing;
  return 0;
}

// The kernels' structure, workgroup by workgroup and tile by tile: the flags with a lane per record and the striding of
// abn_dedup_flags_kernel over `blocks` workgroups (partial: blocks records), the tile counts, their scan, the scatter with
// the rank from the groups' counts.  keep: n bytes; count: tiles + 1 words; order: room for the kept records (at most n)
template <class Keys>
inline DedupCheck dedup_flags_walk(const Keys& keys, long long n, int policy, long long blocks, uint8_t* keep) {
  DedupCheck all;
  for (long long b = 0; b < blocks; ++b) {
    DedupCheck partial;
    for (int t = 0; t < kSortThreads; ++t) {
      DedupCheck lane;
      for (long long i = b * kSortThreads + t; i < n; i += blocks * kSortThreads) dedup_flags_record(keys, i, n, policy, keep, lane);
      partial.add(lane);
    }
    all.add(partial);
  }
  return all;
}

inline long long dedup_compact_walk(const uint8_t* keep, long long n, uint32_t* count, long long* order) {
  const long long tiles = sort_tiles(n);
  for (long long t = 0; t < tiles; ++t) {  // abn_dedup_count_kernel
    uint32_t c = 0;
    for (long long i = t * kSortTile; i < n && i < (t + 1) * kSortTile; ++i) c += keep[i] ? 1u : 0u;
    count[t] = c;
  }
  uint32_t run = 0;
  for (long long t = 0; t <= tiles; ++t) {  // abn_parse_scan_kernel
    const uint32_t v = t < tiles ? count[t] : 0u;
    count[t] = run;
    run += v;
  }
  for (long long t = 0; t < tiles; ++t) {  // abn_dedup_scatter_kernel
    uint32_t group[kSortGroups], before = 0;
    for (int g = 0; g < kSortGroups; ++g) {
      uint32_t c = 0;
      for (long long i = t * kSortTile + g * 64; i < n && i < t * kSortTile + (g + 1) * 64; ++i) c += keep[i] ? 1u : 0u;
      group[g] = before;
      before += c;
    }
    for (int g = 0; g < kSortGroups; ++g) {
      const long long lo = t * kSortTile + g * 64;
      uint32_t in_wave = 0;  // the ballot's popcount below the lane
      for (long long i = lo; i < n && i < lo + 64; ++i)
        if (keep[i]) order[count[t] + group[g] + in_wave++] = i;
    }
  }
  return count[tiles];
}

// one output record from its source: what a lane of abn_dedup_gather_kernel does (n_in: the input's records; an index
// outside them, which no scatter of these kernels gives, copies nothing)
ABN_HOST_DEVICE inline void dedup_gather_record(const SortFlat& in, const uint32_t* order, long long k, long long n_in,
                                                const ParseRecords& out) {
  const uint32_t i = order[k];
  if ((long long)i >= n_in) return;
  out.line[k] = (uint32_t)k;
  out.meta[k] = in.meta[i];
  out.start[k] = in.start[i];
  out.end[k] = in.end[i];
  out.posteriormax[k] = in.posteriormax[i];
  out.meth_lvl[k] = in.meth_lvl[i];
}

#if defined(__HIPCC__) && defined(ABN_SITES_DEDUP_KERNELS)  // (abn_sites_dedup.hip defines it)
// ------------------------------------------------------------------------------------------------ kernels
// grid: at most kSortCheckBlocks workgroups striding over the n records.  keep: n bytes (above: who writes which);
// partial[blockIdx.x * kDedupPartialWords ..] = first descent, bad keys, repeated keys, disagreeing neighbours
template <class Keys>
__global__ void __launch_bounds__(kSortThreads)
abn_dedup_flags_kernel(Keys keys, long long n, int policy, uint8_t* __restrict__ keep, uint32_t* __restrict__ partial) {
  __shared__ uint32_t s_wave[kSortThreads / 64][kDedupPartialWords];
  DedupCheck v;
  for (long long i = (long long)blockIdx.x * kSortThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kSortThreads)
    dedup_flags_record(keys, i, n, policy, keep, v);
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    v.descent = min(v.descent, (uint32_t)__shfl_down(v.descent, d, 64));
    v.bad += __shfl_down(v.bad, d, 64);
    v.repeated += __shfl_down(v.repeated, d, 64);
    v.disagreeing += __shfl_down(v.disagreeing, d, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    uint32_t* s = s_wave[threadIdx.x >> 6];
    s[0] = v.descent, s[1] = v.bad, s[2] = v.repeated, s[3] = v.disagreeing;
  }
  __syncthreads();
  if (threadIdx.x < kDedupPartialWords) {
    const int j = threadIdx.x;
    uint32_t r = s_wave[0][j];
    for (int w = 1; w < kSortThreads / 64; ++w) r = j == 0 ? min(r, s_wave[w][j]) : r + s_wave[w][j];
    partial[(size_t)blockIdx.x * kDedupPartialWords + j] = r;
  }
}

// grid: the tiles.  count[blockIdx.x] = the tile's keep flags
__global__ void __launch_bounds__(kSortThreads)
abn_dedup_count_kernel(const uint8_t* __restrict__ keep, uint32_t n, uint32_t* __restrict__ count) {
  __shared__ uint32_t s_wave[kSortThreads / 64];
  const unsigned long long base = (unsigned long long)blockIdx.x * kSortTile;
  uint32_t kept = 0;  // (the same in every lane of the wavefront)
#pragma unroll
  for (int it = 0; it < kSortItems; ++it) {
    const unsigned long long i = base + (unsigned)(it * kSortThreads) + threadIdx.x;
    kept += (uint32_t)__popcll(__ballot(i < n && keep[i] != 0));
  }
  if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = kept;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t r = 0;
    for (int w = 0; w < kSortThreads / 64; ++w) r += s_wave[w];
    count[blockIdx.x] = r;
  }
}

// grid: the tiles.  off: the scanned counts — off[t] = the records kept in the tiles in front of t.  order has room for
// `room` entries (off[tiles] of them are written, each once)
__global__ void __launch_bounds__(kSortThreads)
abn_dedup_scatter_kernel(const uint8_t* __restrict__ keep, uint32_t n, const uint32_t* __restrict__ off, uint32_t room,
                         uint32_t* __restrict__ order) {
  __shared__ uint32_t s_group[kSortGroups];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long below = (1ull << lane) - 1ull;
  const unsigned long long base = (unsigned long long)blockIdx.x * kSortTile;
  uint32_t in_wave[kSortItems];
  uint32_t mine = 0;  // bit it: this lane's record of item it is kept
#pragma unroll
  for (int it = 0; it < kSortItems; ++it) {
    const unsigned long long i = base + (unsigned)(it * kSortThreads) + threadIdx.x;
    const bool k = i < n && keep[i] != 0;
    const unsigned long long votes = __ballot(k);
    in_wave[it] = (uint32_t)__popcll(votes & below);
    mine |= k ? 1u << it : 0u;
    if (lane == 0) s_group[it * (kSortThreads / 64) + wave] = (uint32_t)__popcll(votes);
  }
  __syncthreads();
  if (threadIdx.x == 0) {  // the groups' counts to their exclusive prefix
    uint32_t before = 0;
    for (int g = 0; g < kSortGroups; ++g) {
      const uint32_t v = s_group[g];
      s_group[g] = before;
      before += v;
    }
  }
  __syncthreads();
  const uint32_t tile_base = off[blockIdx.x];
#pragma unroll
  for (int it = 0; it < kSortItems; ++it) {
    if (!((mine >> it) & 1u)) continue;
    const uint32_t dst = tile_base + s_group[it * (kSortThreads / 64) + wave] + in_wave[it];
    if (dst < room) order[dst] = (uint32_t)(base + (unsigned)(it * kSortThreads) + threadIdx.x);  // (always, for this keep's counts)
  }
}

// grid: ceil(kept / kSortThreads)
__global__ void __launch_bounds__(kSortThreads)
abn_dedup_gather_kernel(SortFlat in, const uint32_t* __restrict__ order, long long kept, long long n_in, ParseRecords out) {
  const long long k = (long long)blockIdx.x * kSortThreads + threadIdx.x;
  if (k < kept) dedup_gather_record(in, order, k, n_in, out);
}
#endif  // kernels

}  // namespace abn
