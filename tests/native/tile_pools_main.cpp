// Stand-alone driver for the serial forms of the region pools (alphabeta_rs_amd/csrc/abn_tiles.hpp: pools), built by
// tests/test_tile_pools_cpu.py plain and with AddressSanitizer + UndefinedBehaviorSanitizer and run directly.  Seeded columns
// — chromosome runs in a shuffled order, starts up to 4294967295, both strands at one start — and seeded pools of intervals
// (overlapping, nested, touching, duplicated, reversed, on absent chromosomes, one interval in several pools, pools without
// any) through tiles_pool_merge, tiles_search_serial, tiles_pool_offsets_serial, tiles_pool_ranges_serial,
// tiles_pool_map_serial and tiles_pool_gather_serial, every array in a heap block of exactly its length (a read or write
// past either end is a report), against a linear scan: column i belongs to pool p when one of p's intervals holds it.  And
// thousands of empty segments in a row between two of one column, with the map searched in windows as the kernel's
// wavefronts search it.  No device.
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "../../alphabeta_rs_amd/csrc/abn_tiles.hpp"

static uint64_t rng_state = 20261021ull;
static uint32_t rnd(uint32_t n) {
  rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
  return n ? (uint32_t)(rng_state >> 33) % n : 0;
}

template <class T>
static std::unique_ptr<T[]> exact(const std::vector<T>& v) {  // a heap block of exactly v's length
  std::unique_ptr<T[]> p(new T[v.size()]);
  if (!v.empty()) std::memcpy(p.get(), v.data(), v.size() * sizeof(T));
  return p;
}

static int fail(const char* what, int it) {
  std::printf("iteration %d: %s\n", it, what);
  return 1;
}

// segments -> columns, offsets, ranges, map, all in exact blocks; compares src and the ranges with want_src / want_first
static int check_chain(const abn::PoolSegments& seg, int n_pools, const uint32_t* start, const long long* run_begin,
                       const long long* run_end, const std::vector<long long>& want_src,
                       const std::vector<long long>& want_begin, std::vector<long long>* src_out, size_t* empties, int it) {
  const long long S = (long long)seg.size();
  const auto sc = exact(seg.chromosome);
  const auto ss = exact(seg.start), se = exact(seg.end), first = exact(seg.seg_first);
  std::unique_ptr<long long[]> cb(new long long[(size_t)S]), ce(new long long[(size_t)S]), off(new long long[(size_t)S + 1]);
  std::unique_ptr<long long[]> begin(new long long[(size_t)n_pools]), end(new long long[(size_t)n_pools]);
  abn::tiles_search_serial(start, run_begin, run_end, S, sc.get(), ss.get(), se.get(), cb.get(), ce.get());
  abn::tiles_pool_offsets_serial(cb.get(), ce.get(), S, off.get());
  abn::tiles_pool_ranges_serial(off.get(), first.get(), n_pools, begin.get(), end.get());
  const long long pooled = off[(size_t)S];
  if (pooled != (long long)want_src.size()) return fail("the pooled columns' number", it);
  std::unique_ptr<long long[]> src(new long long[(size_t)pooled]);
  abn::tiles_pool_map_serial(off.get(), S, cb.get(), src.get());
  for (long long j = 0; j < pooled; ++j)
    if (src[(size_t)j] != want_src[(size_t)j]) return fail("a pooled column's source", it);
  for (int p = 0; p < n_pools; ++p)
    if (begin[(size_t)p] != want_begin[(size_t)p] || end[(size_t)p] != want_begin[(size_t)p + 1]) return fail("a pool's range", it);
  // the map as a wavefront searches it: the segments of the first and last of 64 columns, every column inside that window
  for (long long w = 0; w < pooled; w += 64) {
    const long long last = std::min(w + 63, pooled - 1);
    const long long lo = abn::tiles_pool_segment_of(off.get(), 0, S - 1, w), hi = abn::tiles_pool_segment_of(off.get(), lo, S - 1, last);
    if (ce[(size_t)lo] == cb[(size_t)lo] || ce[(size_t)hi] == cb[(size_t)hi]) return fail("a column in an empty segment", it);
    for (long long j = w; j <= last; ++j)
      if (abn::tiles_pool_map_lane(off.get(), lo, hi, cb.get(), j) != src[(size_t)j]) return fail("the map inside a window", it);
    // ... and on a copy of the window alone, indices from 0, as the lanes read it from LDS
    std::vector<long long> window(off.get() + lo, off.get() + hi + 2);
    const auto xw = exact(window);
    for (long long j = w; j <= last; ++j)
      if (abn::tiles_pool_map_lane(xw.get(), 0, hi - lo, cb.get() + lo, j) != src[(size_t)j]) return fail("the map on a window's copy", it);
  }
  for (long long i = 0; i < S; ++i) *empties += cb[(size_t)i] == ce[(size_t)i];
  src_out->assign(src.get(), src.get() + pooled);
  return 0;
}

int main() {
  size_t columns = 0, intervals = 0, segments = 0, empties = 0, empty_pools = 0, pooled_columns = 0, shared = 0, joined = 0;
  for (int it = 0; it < 60; ++it) {
    // the columns: runs of chromosomes drawn without repeat, in the order drawn
    const int n_runs = it == 0 ? 0 : 1 + (int)rnd(5);
    std::vector<int32_t> chrom;
    std::vector<uint32_t> start;
    std::vector<uint8_t> strand;
    std::vector<int> used;
    for (int r = 0; r < n_runs; ++r) {
      int c;
      do c = (int)rnd(4) == 0 ? 256 + (int)rnd(2) : (int)rnd(12);
      while (std::find(used.begin(), used.end(), c) != used.end());
      used.push_back(c);
      const long long len = rnd(4) == 0 ? 1 : 1 + rnd(300);
      const bool high = rnd(3) == 0;
      uint64_t pos = high ? 4294967295ull - 40ull * (uint64_t)len : rnd(1000);
      for (long long k = 0; k < len; ++k) {
        const bool pair = k > 0 && strand.back() == 0 && chrom.back() == c && rnd(8) == 0;
        if (!pair) pos += 1 + rnd(39);
        if (high && k == len - 1 && !pair) pos = 4294967295ull;
        chrom.push_back(c), start.push_back((uint32_t)pos), strand.push_back(pair ? 1 : 0);
      }
    }
    const long long n_columns = (long long)chrom.size();
    columns += (size_t)n_columns;
    const auto xchrom = exact(chrom);
    const auto xstart = exact(start);
    const auto xstrand = exact(strand);
    const abn::CommonSites keys{xchrom.get(), xstart.get(), xstart.get(), xstrand.get()};
    std::unique_ptr<long long[]> run_begin(new long long[abn::kCommonChroms]), run_end(new long long[abn::kCommonChroms]);
    std::vector<abn::TileRun> runs;
    abn::CommonRefusal refusal{0, -1, -1};
    if (!abn::tiles_runs_serial(keys, n_columns, run_begin.get(), run_end.get(), &runs, &refusal)) return fail("refused", it);

    // the pools' intervals, in no order
    const int n_pools = 1 + (int)rnd(6);
    std::vector<int32_t> ic, ip;
    std::vector<long long> is, ie;
    const int K = it == 1 ? 0 : (int)rnd(120);
    for (int k = 0; k < K; ++k) {
      const int kind = (int)rnd(8);
      const int c = n_runs && kind != 0 ? used[rnd((uint32_t)n_runs)] : (int)rnd(258);
      long long a, b;
      if (k > 0 && kind == 1) {  // an earlier interval once more, often in another pool
        const size_t e = rnd((uint32_t)k);
        ic.push_back(ic[e]), is.push_back(is[e]), ie.push_back(ie[e]), ip.push_back((int32_t)rnd((uint32_t)n_pools));
        shared += ip.back() != ip[e];
        continue;
      }
      if (n_columns && kind >= 3) {
        const abn::TileRun* run = nullptr;
        for (const auto& r : runs)
          if (r.chromosome == c) run = &r;
        const long long i = run->first + rnd((uint32_t)run->count), j = run->first + rnd((uint32_t)run->count);
        a = (long long)start[(size_t)std::min(i, j)] + (long long)rnd(3) - 1;
        b = (long long)start[(size_t)std::max(i, j)] + (long long)rnd(3);
        if (a < 0) a = 0;
        if (kind == 6 && !is.empty()) a = ie.back();  // touches the interval before it, if that is of its chromosome and pool
        if (kind == 7) std::swap(a, b);
      } else if (kind == 2) {
        a = 0, b = abn::kTilesPosEnd;
      } else {
        a = rnd(100000), b = a + rnd(1000);
      }
      a = std::min(a, abn::kTilesPosEnd), b = std::min(b, abn::kTilesPosEnd);
      if (!abn::tiles_interval_valid(c, a, b)) return fail("a valid interval is called invalid", it);
      ic.push_back(c), is.push_back(a), ie.push_back(b);
      ip.push_back(kind == 6 && !ip.empty() ? ip.back() : (int32_t)rnd((uint32_t)(n_pools > 1 ? n_pools - 1 : 1)));  // the last pool
    }                                                                                                              // often stays empty
    intervals += ic.size();
    const auto xic = exact(ic), xip = exact(ip);
    const auto xis = exact(is), xie = exact(ie);
    abn::PoolSegments seg;
    abn::tiles_pool_merge(runs.data(), n_runs, (long long)ic.size(), xic.get(), xis.get(), xie.get(), xip.get(), n_pools, &seg);
    segments += seg.size();
    // the segments: inside a pool in run order and ascending, disjoint and not touching; every kept interval inside one
    if (seg.seg_first.size() != (size_t)n_pools + 1 || seg.seg_first[0] != 0 || seg.seg_first.back() != (long long)seg.size())
      return fail("seg_first", it);
    for (int p = 0; p < n_pools; ++p)
      for (long long i = seg.seg_first[(size_t)p]; i < seg.seg_first[(size_t)p + 1]; ++i) {
        if (seg.pool[(size_t)i] != p || seg.end[(size_t)i] <= seg.start[(size_t)i]) return fail("a segment's pool or bounds", it);
        if (i == seg.seg_first[(size_t)p]) continue;
        int ra = -1, rb = -1;
        for (int r = 0; r < n_runs; ++r) {
          if (runs[(size_t)r].chromosome == seg.chromosome[(size_t)i - 1]) ra = r;
          if (runs[(size_t)r].chromosome == seg.chromosome[(size_t)i]) rb = r;
        }
        if (ra < 0 || rb < 0 || ra > rb || (ra == rb && seg.start[(size_t)i] <= seg.end[(size_t)i - 1]))
          return fail("the segments' order", it);
      }
    joined += ic.size() > seg.size();
    // the linear scan
    std::vector<long long> want_src, want_begin(1, 0);
    for (int p = 0; p < n_pools; ++p) {
      for (long long i = 0; i < n_columns; ++i) {
        bool in = false;
        for (size_t k = 0; k < ic.size() && !in; ++k)
          in = ip[k] == p && ic[k] == chrom[(size_t)i] && is[k] <= (long long)start[(size_t)i] && (long long)start[(size_t)i] < ie[k];
        if (in) want_src.push_back(i);
      }
      empty_pools += (long long)want_src.size() == want_begin.back();
      want_begin.push_back((long long)want_src.size());
    }
    std::vector<long long> src;
    if (check_chain(seg, n_pools, xstart.get(), run_begin.get(), run_end.get(), want_src, want_begin, &src, &empties, it)) return 1;
    pooled_columns += src.size();

    // the gather
    const int n = 1 + (int)rnd(3);
    const long long code_stride = (n_columns + 15) / 16 * 16, pooled = (long long)src.size(), pstride = (pooled + 15) / 16 * 16;
    std::vector<uint8_t> code((size_t)(n * code_stride), 0x7f);
    std::vector<double> level((size_t)(n * n_columns));
    for (int s = 0; s < n; ++s)
      for (long long i = 0; i < n_columns; ++i) {
        code[(size_t)(s * code_stride + i)] = (uint8_t)(rnd(3) | (rnd(3) ? abn::kCodeCounted : 0x80));
        level[(size_t)(s * n_columns + i)] = rnd(4) ? rnd(1000) / 1000.0 : -0.0;
      }
    const auto xcode = exact(code);
    const auto xlevel = exact(level);
    const auto xsrc = exact(src);
    std::unique_ptr<uint8_t[]> pcode(new uint8_t[(size_t)(n * pstride)]);
    std::unique_ptr<double[]> plevel(new double[(size_t)(n * pooled)]);
    std::memset(pcode.get(), 0x55, (size_t)(n * pstride));
    abn::tiles_pool_gather_serial(xcode.get(), code_stride, xlevel.get(), n_columns, n, xsrc.get(), pooled, pcode.get(), pstride,
                                  plevel.get());
    for (int s = 0; s < n; ++s) {
      for (long long j = 0; j < pooled; ++j)
        if (pcode[(size_t)(s * pstride + j)] != code[(size_t)(s * code_stride + src[(size_t)j])] ||
            std::memcmp(&plevel[(size_t)(s * pooled + j)], &level[(size_t)(s * n_columns + src[(size_t)j])], 8) != 0)
          return fail("a gathered byte or level", it);
      for (long long j = pooled; j < pstride; ++j)
        if (pcode[(size_t)(s * pstride + j)] != 0x55) return fail("the gather wrote behind the pooled columns", it);
    }
  }
  // 5000 empty segments in a row between two of one column: one run of 600 columns 10 bp apart, the empties between two sites
  {
    std::vector<int32_t> chrom(600, 3);
    std::vector<uint32_t> start;
    std::vector<uint8_t> strand(600, 0);
    for (uint32_t k = 0; k < 600; ++k) start.push_back(k < 300 ? 10 * k : 1000000 + 10 * k);
    const auto xchrom = exact(chrom);
    const auto xstart = exact(start);
    const auto xstrand = exact(strand);
    std::unique_ptr<long long[]> run_begin(new long long[abn::kCommonChroms]), run_end(new long long[abn::kCommonChroms]);
    std::vector<abn::TileRun> runs;
    abn::CommonRefusal refusal{0, -1, -1};
    if (!abn::tiles_runs_serial(abn::CommonSites{xchrom.get(), xstart.get(), xstart.get(), xstrand.get()}, 600, run_begin.get(),
                                run_end.get(), &runs, &refusal))
      return fail("refused", -1);
    std::vector<int32_t> ic{3, 3}, ip{0, 0};
    std::vector<long long> is{start[299], start[300]}, ie{start[299] + 1, start[300] + 1};
    for (long long k = 0; k < 5000; ++k) ic.push_back(3), ip.push_back(0), is.push_back(5000 + 2 * k), ie.push_back(5001 + 2 * k);
    const auto xic = exact(ic), xip = exact(ip);
    const auto xis = exact(is), xie = exact(ie);
    abn::PoolSegments seg;
    abn::tiles_pool_merge(runs.data(), 1, (long long)ic.size(), xic.get(), xis.get(), xie.get(), xip.get(), 1, &seg);
    if (seg.size() != 5002) return fail("the empty segments are merged or lost", -1);
    std::vector<long long> src;
    size_t e = 0;
    if (check_chain(seg, 1, xstart.get(), run_begin.get(), run_end.get(), {299, 300}, {0, 2}, &src, &e, -1)) return 1;
    if (e != 5000) return fail("the empty segments' number", -1);
  }
  if (!columns || !intervals || !segments || !empties || !empty_pools || !pooled_columns || !shared || !joined) {
    std::printf("the cases miss a pattern: %zu %zu %zu %zu %zu %zu %zu %zu\n", columns, intervals, segments, empties, empty_pools,
                pooled_columns, shared, joined);
    return 1;
  }
  std::printf("tile pools serial forms ok: %zu columns, %zu intervals in %zu segments (%zu empty), %zu pooled columns, %zu empty pools\n",
              columns, intervals, segments, empties, pooled_columns, empty_pools);
  return 0;
}
