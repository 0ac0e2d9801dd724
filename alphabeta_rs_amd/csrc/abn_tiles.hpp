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
// Every output element has one writer, a plain store; no atomics here.
//
// The arithmetic and every step in its serial form compile without a HIP header: the host library (host_capi.cpp) and
// tests/native/tiles_main.cpp include this file as it is.
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
#endif  // kernels

}  // namespace abn
