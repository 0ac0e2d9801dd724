// Genomic tiles over resident, aligned methylomes (abn_tiles_*): every tile — a fixed bin of the genome or a row of a
// user's region list — gets the columns of the packed code matrix it covers and, per sample, its own rc_meth_lvl fold, so
// that each tile is a pedigree of its own (src/pedigree.rs:147-172 and :210-261 over the tile's sites alone; the region
// rows src/cli/metaprofile.rs:50-72 anticipates).
//
// The COLUMNS are the samples' sites after the alignment (abn_sites_common.hpp, abn_sites_union.hpp, or none: the
// reference's assumption, src/pedigree.rs:240, that site k is the same site in every sample).  Column k has one key
// (chromosome, start) for all samples; the columns of a chromosome form one contiguous RUN, ascending in start (the order
// checks of abn_sites_common.hpp: runs, ends), and the runs may come in any order.  A TILE is an interval (chromosome,
// start, end), half-open on the site's `start` — the pos = start of window placement; the strand is no part of it, so both
// strands' sites at one position share a tile — and therefore a contiguous column range [begin, end).
//
//   search  a lane per interval: its chromosome's run from the table in LDS, two lower bounds on `start` inside it.
//           begin = end (an empty tile) for a chromosome without a run, for end <= start and behind the last site.
//           Positions are compared in 64 bits: start and end lie in [0, 2^32], so k * step + size never wraps.
//   fold    a wavefront per (sample, tile): codes_fold_wave (abn_codes.hpp) over the tile's columns of the sample's merged
//           bytes and levels — the chain s = s + x from +0.0 in file order, +0.0 for an uncounted site, the exactness
//           argument of abn_codes.hpp — so level_sum_kept has the bits of the host loop run over that tile's sites alone.
//           n x T independent chains where the whole-sample fold has n.  `begin` is aligned to nothing: the loads are
//           byte and double loads at begin + lane, the index clamped to the tile's last column.
//
//   pools   a set of intervals as ONE tile — a class of an annotation: its non-contiguous columns made a contiguous range of
//           a pooled matrix (merge, offsets, map, gather: the section "pools" below), which the same fold and scan take.
//
// Every output element has one writer, a plain store; no atomics here.
//
// The arithmetic and every step in its serial form compile without a HIP header: the host library (host_capi.cpp),
// tests/native/tiles_main.cpp and tests/native/tile_pools_main.cpp include this file as it is.
#pragma once
#include <algorithm>

#include "abn_codes.hpp"
#include "abn_sites_common.hpp"

namespace abn {

constexpr int kTilesThreads = 256;              // the search kernel's workgroup
constexpr long long kTilesPosEnd = 1LL << 32;   // the highest interval bound: behind every site's start

struct TileRun {  // a chromosome run of the columns, as the host reads it (abn_tiles_runs)
  int32_t chromosome;
  long long first, count;
  uint32_t last_start;  // the start of the run's last column
};

ABN_HOST_DEVICE inline bool tiles_interval_valid(int32_t chromosome, long long start, long long end) {
  return chromosome >= 0 && chromosome < kCommonChroms && start >= 0 && start <= kTilesPosEnd && end >= 0 &&
         end <= kTilesPosEnd;
}

// the first column of [lo, hi) whose start is not below pos (hi if none); pos in 64 bits
ABN_HOST_DEVICE inline long long tiles_lower_bound(const uint32_t* start, long long lo, long long hi, long long pos) {
  while (lo < hi) {
    const long long mid = lo + (hi - lo) / 2;
    if ((long long)start[mid] < pos) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// One interval -> its column range.  run_begin / run_end [kCommonChroms]: the tables of the runs and ends passes over the
// columns (a chromosome without a run: begin kCommonNone, end 0).  An empty tile of a chromosome without a run is [0, 0).
ABN_HOST_DEVICE inline void tiles_search_lane(const uint32_t* start, const long long* run_begin, const long long* run_end,
                                              int32_t chromosome, long long pos, long long pos_end, long long* begin,
                                              long long* end) {
  const long long lo = run_begin[chromosome], hi = run_end[chromosome];
  if (lo >= hi) {
    *begin = *end = 0;
    return;
  }
  const long long b = tiles_lower_bound(start, lo, hi, pos);
  *begin = b;
  *end = pos_end <= pos ? b : tiles_lower_bound(start, b, hi, pos_end);
}

// ---- the serial forms
// the run table, in run order, from the tables of the runs and ends passes and every chromosome's last start (what
// abn_tiles_last_kernel leaves)
inline void tiles_runs_from_tables(const long long* run_begin, const long long* run_end, const uint32_t* last_start,
                                   std::vector<TileRun>* runs) {
  runs->clear();
  for (int c = 0; c < kCommonChroms; ++c)
    if (run_begin[c] < run_end[c]) runs->push_back(TileRun{c, run_begin[c], run_end[c] - run_begin[c], last_start[c]});
  std::sort(runs->begin(), runs->end(), [](const TileRun& a, const TileRun& b) { return a.first < b.first; });
}

// The run tables of the columns' keys (one sample: the runs and ends passes of abn_sites_common.hpp, with their refusals)
// and the run table.  Returns false with *refusal set for keys that are not well ordered.
inline bool tiles_runs_serial(const CommonSites& keys, long long n_columns, long long* run_begin, long long* run_end,
                              std::vector<TileRun>* runs, CommonRefusal* refusal) {
  const long long site_off[2] = {0, n_columns};
  long long err[kCommonErrs] = {kCommonNone, kCommonNone, kCommonNone, kCommonNone};
  for (int c = 0; c < kCommonChroms; ++c) run_begin[c] = kCommonNone, run_end[c] = 0;
  for (long long i = 0; i < n_columns; ++i) common_runs_lane(keys, site_off, 0, i, run_begin, err);
  for (long long i = 0; i < n_columns; ++i) common_ends_lane(keys, site_off, 0, i, run_begin, run_end, err);
  *refusal = common_refusal(err, kCommonSplitRun, kCommonBadKey, site_off, 1);
  if (refusal->kind) return false;
  uint32_t last_start[kCommonChroms];
  for (int c = 0; c < kCommonChroms; ++c) last_start[c] = run_begin[c] < run_end[c] ? keys.start[run_end[c] - 1] : 0u;
  tiles_runs_from_tables(run_begin, run_end, last_start, runs);
  return true;
}

// The fixed tiles of abn_tiles_set_fixed: for every run in run order the tiles k = 0 .. ceil((last_start + 1) / step) - 1,
// [k step, k step + size), the end capped at 2^32 (no site lies behind it).  step 0: size.  Returns the number of tiles (-1:
// size <= 0 or step < 0); with null outputs it only counts.
inline long long tiles_fixed_intervals(const TileRun* runs, int n_runs, long long size, long long step, int32_t* chromosome,
                                       long long* start, long long* end) {
  if (size <= 0 || step < 0) return -1;
  if (step == 0) step = size;
  long long t = 0;
  for (int r = 0; r < n_runs; ++r) {
    const long long tiles = (long long)runs[r].last_start / step + 1;  // ceil((last_start + 1) / step), for any step
    if (chromosome)
      for (long long k = 0; k < tiles; ++k) {
        chromosome[t + k] = runs[r].chromosome;
        start[t + k] = k * step;  // (below 2^32: k step <= last_start)
        end[t + k] = size > kTilesPosEnd - k * step ? kTilesPosEnd : k * step + size;
      }
    t += tiles;
  }
  return t;
}

inline void tiles_search_serial(const uint32_t* start, const long long* run_begin, const long long* run_end, long long T,
                                const int32_t* chromosome, const long long* pos, const long long* pos_end,
                                long long* begin, long long* end) {
  for (long long t = 0; t < T; ++t)
    tiles_search_lane(start, run_begin, run_end, chromosome[t], pos[t], pos_end[t], &begin[t], &end[t]);
}

// sum, kept [n x T]: sample s's merged bytes at code + s code_stride, its levels at level + s n_columns
inline void tiles_fold_serial(const uint8_t* code, long long code_stride, const double* level, long long n_columns, int n,
                              long long T, const long long* begin, const long long* end, double* sum, long long* kept) {
  for (int s = 0; s < n; ++s)
    for (long long t = 0; t < T; ++t)
      codes_fold_serial(code + s * code_stride + begin[t], level + s * n_columns + begin[t], end[t] - begin[t],
                        &sum[s * T + t], &kept[s * T + t]);
}

// the limits of one handle's matrix of n rows of `columns` sites, stride_bytes each: the grids of the pack (a lane per dword)
// and of the passes with a lane per column
inline bool tiles_matrix_fits(int n, long long columns, long long stride_bytes) {
  return ((long long)n * (stride_bytes / 4) + kCodesThreads - 1) / kCodesThreads <= 0x7fffffffLL &&
         (columns + kCommonThreads - 1) / kCommonThreads <= 0x7fffffffLL;
}

// ------------------------------------------------------------------------------------------------ pools
// A POOL is a set of intervals that belong together — every gene, every TE, the segments of one chromatin state: the one
// rate per annotation class the AlphaBeta analyses report, where a tile is one row of the list.  Its columns are the columns
// whose (chromosome, start) lies in at least one of its intervals, each once, in ascending column order; gathered side by
// side they are a contiguous range of a POOLED matrix, and from there on a pool is a tile: the same fold, the same scan.
//
//   merge    on the host, pool by pool: the chromosomes in the RUN order of the columns (not in key order), one without a run
//            dropped, intervals with end <= start dropped, the rest sorted by (start, end), overlapping or touching ones
//            merged.  A pool's SEGMENTS are therefore disjoint and ascend in column space; seg_first[p] is pool p's first.
//   search   a segment's column range [col_begin, col_end) is tiles_search_lane's, unchanged; a segment may be empty.
//   offsets  seg_off [S + 1]: the exclusive prefix of the segments' lengths in segment order, in 64 bits; pool p owns the
//            pooled columns [seg_off[seg_first[p]], seg_off[seg_first[p + 1]]).
//   map      a lane per pooled column j: src[j] = col_begin[i] + (j - seg_off[i]), i the LAST segment with seg_off[i] <= j
//            (an upper bound, so the empty segments in front of it are passed over).
//   gather   a lane per (sample, pooled column): the merged byte and the level of src[j], into arrays laid out as the
//            handle's own (rows of pooled_code_stride bytes, of pooled_columns levels), which the pack and the fold take.
struct PoolSegments {
  std::vector<int32_t> pool, chromosome;  // [S] in segment order: pool by pool, inside one in column order
  std::vector<long long> start, end;
  std::vector<long long> seg_first;       // [n_pools + 1]
  size_t size() const { return pool.size(); }
};

// interval k = (chromosome, start, end)[k], valid (tiles_interval_valid), belongs to pool[k] in [0, n_pools)
inline void tiles_pool_merge(const TileRun* runs, int n_runs, long long n_intervals, const int32_t* chromosome,
                             const long long* start, const long long* end, const int32_t* pool, int32_t n_pools,
                             PoolSegments* out) {
  int rank[kCommonChroms];
  for (int c = 0; c < kCommonChroms; ++c) rank[c] = -1;
  for (int r = 0; r < n_runs; ++r) rank[runs[r].chromosome] = r;
  std::vector<long long> order;
  for (long long k = 0; k < n_intervals; ++k)
    if (end[k] > start[k] && rank[chromosome[k]] >= 0) order.push_back(k);
  std::sort(order.begin(), order.end(), [&](long long a, long long b) {
    if (pool[a] != pool[b]) return pool[a] < pool[b];
    if (chromosome[a] != chromosome[b]) return rank[chromosome[a]] < rank[chromosome[b]];
    if (start[a] != start[b]) return start[a] < start[b];
    return end[a] < end[b];
  });
  *out = PoolSegments{};
  out->seg_first.assign((size_t)n_pools + 1, 0);
  for (long long k : order) {
    const bool joins = !out->pool.empty() && out->pool.back() == pool[k] && out->chromosome.back() == chromosome[k] &&
                       start[k] <= out->end.back();  // overlaps the segment, or touches it
    if (joins) {
      out->end.back() = std::max(out->end.back(), end[k]);
      continue;
    }
    out->pool.push_back(pool[k]), out->chromosome.push_back(chromosome[k]);
    out->start.push_back(start[k]), out->end.push_back(end[k]);
    ++out->seg_first[(size_t)pool[k] + 1];
  }
  for (size_t p = 0; p < (size_t)n_pools; ++p) out->seg_first[p + 1] += out->seg_first[p];
}

// The last segment of [lo, hi] whose offset is not above j; seg_off[lo] <= j < seg_off[hi + 1].  (The kernel's lanes call it
// on a window of seg_off, from LDS where it fits.)
ABN_HOST_DEVICE inline long long tiles_pool_segment_of(const long long* seg_off, long long lo, long long hi, long long j) {
  long long a = lo + 1, b = hi + 1;  // the first offset above j lies in [a, b]
  while (a < b) {
    const long long mid = a + (b - a) / 2;
    if (seg_off[mid] > j) b = mid;
    else a = mid + 1;
  }
  return a - 1;
}

// pooled column j -> its source column; the segment is searched in [lo, hi] (the whole list: 0, S - 1)
ABN_HOST_DEVICE inline long long tiles_pool_map_lane(const long long* seg_off, long long lo, long long hi,
                                                     const long long* col_begin, long long j) {
  const long long i = tiles_pool_segment_of(seg_off, lo, hi, j);
  return col_begin[i] + (j - seg_off[i]);
}

// sample s's pooled column j from its source column: the merged byte and the level.  code / level: the handle's arrays
// (rows of code_stride bytes, of n_columns levels); pcode / plevel: the pooled ones (pcode_stride, pooled)
ABN_HOST_DEVICE inline void tiles_pool_gather_lane(const uint8_t* code, long long code_stride, const double* level,
                                                   long long n_columns, long long s, long long j, long long src,
                                                   uint8_t* pcode, long long pcode_stride, double* plevel,
                                                   long long pooled) {
  pcode[s * pcode_stride + j] = code[s * code_stride + src];
  plevel[s * pooled + j] = level[s * n_columns + src];
}

// ---- their serial forms
inline void tiles_pool_offsets_serial(const long long* col_begin, const long long* col_end, long long S, long long* seg_off) {
  long long run = 0;
  for (long long i = 0; i < S; ++i) {
    seg_off[i] = run;
    run += col_end[i] - col_begin[i];
  }
  seg_off[S] = run;
}

// pool p's range of pooled columns
inline void tiles_pool_ranges_serial(const long long* seg_off, const long long* seg_first, long long n_pools, long long* begin,
                                     long long* end) {
  for (long long p = 0; p < n_pools; ++p) begin[p] = seg_off[seg_first[p]], end[p] = seg_off[seg_first[p + 1]];
}

inline void tiles_pool_map_serial(const long long* seg_off, long long S, const long long* col_begin, long long* src) {
  for (long long j = 0; j < seg_off[S]; ++j) src[j] = tiles_pool_map_lane(seg_off, 0, S - 1, col_begin, j);
}

inline void tiles_pool_gather_serial(const uint8_t* code, long long code_stride, const double* level, long long n_columns,
                                     int n, const long long* src, long long pooled, uint8_t* pcode, long long pcode_stride,
                                     double* plevel) {
  for (int s = 0; s < n; ++s)
    for (long long j = 0; j < pooled; ++j)
      tiles_pool_gather_lane(code, code_stride, level, n_columns, s, j, src[j], pcode, pcode_stride, plevel, pooled);
}

#if defined(__HIPCC__) && defined(ABN_TILES_KERNELS)  // (abn_tiles.hip defines it)
// ------------------------------------------------------------------------------------------------ kernels
// grid: ceil(kCommonChroms / kTilesThreads); last_start[c] = the start of the last column of chromosome c's run
__global__ void __launch_bounds__(kTilesThreads)
abn_tiles_last_kernel(const uint32_t* __restrict__ start, const long long* __restrict__ run_begin,
                      const long long* __restrict__ run_end, uint32_t* __restrict__ last_start) {
  const int c = blockIdx.x * kTilesThreads + threadIdx.x;
  if (c >= kCommonChroms) return;
  const long long lo = run_begin[c], hi = run_end[c];
  last_start[c] = lo < hi ? start[hi - 1] : 0u;
}

// grid: ceil(T / kTilesThreads); the run tables [kCommonChroms] go to LDS once per workgroup
__global__ void __launch_bounds__(kTilesThreads)
abn_tiles_search_kernel(const uint32_t* __restrict__ start, const long long* __restrict__ run_begin,
                        const long long* __restrict__ run_end, long long T, const int32_t* __restrict__ chromosome,
                        const long long* __restrict__ pos, const long long* __restrict__ pos_end,
                        long long* __restrict__ begin, long long* __restrict__ end) {
  __shared__ long long s_begin[kCommonChroms], s_end[kCommonChroms];
  for (int c = threadIdx.x; c < kCommonChroms; c += kTilesThreads) s_begin[c] = run_begin[c], s_end[c] = run_end[c];
  __syncthreads();
  const long long t = (long long)blockIdx.x * kTilesThreads + threadIdx.x;
  if (t >= T) return;
  long long b, e;
  tiles_search_lane(start, s_begin, s_end, chromosome[t], pos[t], pos_end[t], &b, &e);
  begin[t] = b;
  end[t] = e;
}

// grid: (T, n_samples) workgroups of one wavefront; sum, kept [n_samples x T].  The tile's columns lie inside the
// sample's arrays (0 <= begin <= end <= n_columns), and codes_fold_wave reads none but them.
__global__ void __launch_bounds__(kCodesWave)
abn_tiles_fold_kernel(const uint8_t* __restrict__ code, long long code_stride, const double* __restrict__ level,
                      long long n_columns, long long T, const long long* __restrict__ begin,
                      const long long* __restrict__ end, double* __restrict__ sum, long long* __restrict__ kept) {
  const long long t = blockIdx.x, s = blockIdx.y;
  const int lane = threadIdx.x;
  const long long b = begin[t];
  double acc;
  long long count;
  codes_fold_wave(code + s * code_stride + b, level + s * n_columns + b, end[t] - b, lane, acc, count);
  if (lane == 0) {
    sum[s * T + t] = acc;
    kept[s * T + t] = count;
  }
}

// ---- pools
constexpr int kPoolWindow = 128;  // the offsets a wavefront of the map kernel keeps in LDS (4 wavefronts: 4 KiB)

// one workgroup: seg_off[0 .. S) = the exclusive prefix of the segments' lengths, in 64 bits, the sum at seg_off[S] —
// abn_common_scan_kernel's two levels: every lane its slice of the segments serially, the 256 sums by Hillis-Steele in LDS
__global__ void __launch_bounds__(kTilesThreads)
abn_tiles_pool_offsets_kernel(const long long* __restrict__ col_begin, const long long* __restrict__ col_end, long long S,
                              long long* __restrict__ seg_off) {
  __shared__ long long s_part[kTilesThreads];
  const long long per = (S + kTilesThreads - 1) / kTilesThreads;
  const long long lo = min((long long)threadIdx.x * per, S), hi = min(lo + per, S);
  long long sum = 0;
  for (long long i = lo; i < hi; ++i) sum += col_end[i] - col_begin[i];
  s_part[threadIdx.x] = sum;
  __syncthreads();
  for (int d = 1; d < kTilesThreads; d <<= 1) {  // inclusive
    const long long up = threadIdx.x >= (unsigned)d ? s_part[threadIdx.x - d] : 0;
    __syncthreads();
    s_part[threadIdx.x] += up;
    __syncthreads();
  }
  long long run = s_part[threadIdx.x] - sum;
  for (long long i = lo; i < hi; ++i) {
    seg_off[i] = run;
    run += col_end[i] - col_begin[i];
  }
  if (threadIdx.x == kTilesThreads - 1) seg_off[S] = s_part[threadIdx.x];
}

// grid: ceil(n_pools / kTilesThreads); pool p's range of pooled columns, where the fold reads its tiles' ranges
__global__ void __launch_bounds__(kTilesThreads)
abn_tiles_pool_ranges_kernel(const long long* __restrict__ seg_off, const long long* __restrict__ seg_first, long long n_pools,
                             long long* __restrict__ begin, long long* __restrict__ end) {
  const long long p = (long long)blockIdx.x * kTilesThreads + threadIdx.x;
  if (p >= n_pools) return;
  begin[p] = seg_off[seg_first[p]];
  end[p] = seg_off[seg_first[p + 1]];
}

// grid: ceil(pooled / kTilesThreads), pooled = seg_off[S] > 0; src[j] = pooled column j's source column.  A wavefront's 64
// columns ascend, so their segments lie between its first column's and its last's: those two are searched in the whole list
// (the same two probes in every lane: one broadcast load per step), and every lane then searches that window alone — from
// LDS where its offsets fit (kPoolWindow), else in seg_off itself, which is what a wavefront over thousands of empty
// segments does.  Either way the upper bound passes over the empty segments.
__global__ void __launch_bounds__(kTilesThreads)
abn_tiles_pool_map_kernel(const long long* __restrict__ seg_off, long long S, const long long* __restrict__ col_begin,
                          long long pooled, long long* __restrict__ src) {
  __shared__ long long s_off[kTilesThreads / 64][kPoolWindow];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long j = (long long)blockIdx.x * kTilesThreads + threadIdx.x, first = j - lane;
  const bool live = first < pooled;  // (wave-uniform)
  long long lo = 0, hi = 0;
  if (live) {
    const long long last = min(first + 63, pooled - 1);
    lo = tiles_pool_segment_of(seg_off, 0, S - 1, first);
    hi = tiles_pool_segment_of(seg_off, lo, S - 1, last);
  }
  const long long span = hi - lo + 2;  // the offsets lo .. hi + 1
  const bool fits = live && span <= kPoolWindow;
  if (fits)
    for (long long k = lane; k < span; k += 64) s_off[wave][k] = seg_off[lo + k];
  __syncthreads();
  if (j >= pooled) return;
  if (fits) src[j] = tiles_pool_map_lane(s_off[wave], 0, hi - lo, col_begin + lo, j);
  else src[j] = tiles_pool_map_lane(seg_off, lo, hi, col_begin, j);
}

// grid: (ceil(pooled / kTilesThreads), n_samples); a lane per (sample, pooled column): src read once, the sample's merged byte
// and level of that column to the pooled arrays — consecutive lanes, consecutive bytes and doubles, one writer each
__global__ void __launch_bounds__(kTilesThreads)
abn_tiles_pool_gather_kernel(const uint8_t* __restrict__ code, long long code_stride, const double* __restrict__ level,
                             long long n_columns, const long long* __restrict__ src, long long pooled,
                             uint8_t* __restrict__ pcode, long long pcode_stride, double* __restrict__ plevel) {
  const long long j = (long long)blockIdx.x * kTilesThreads + threadIdx.x;
  if (j >= pooled) return;
  tiles_pool_gather_lane(code, code_stride, level, n_columns, blockIdx.y, j, src[j], pcode, pcode_stride, plevel, pooled);
}
#endif  // kernels

}  // namespace abn
