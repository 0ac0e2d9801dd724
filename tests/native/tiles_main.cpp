// Stand-alone driver for the serial forms of the genomic tiles (alphabeta_rs_amd/csrc/abn_tiles.hpp), built by
// tests/test_tiles_cpu.py plain and with AddressSanitizer + UndefinedBehaviorSanitizer and run directly.  Seeded columns —
// chromosome runs in a shuffled order, starts up to 4294967295, both strands at one start, runs of one column, no column
// at all — and seeded tiles (inside a run, over its ends, empty, reversed, absent chromosomes, bounds 0 and 2^32) through
// tiles_runs_serial, tiles_search_serial, tiles_fold_serial and tiles_fixed_intervals, every array in a heap block of
// exactly its length (a read or write past either end is a report), against a linear scan for the column range, a plain
// `if counted` fold and the tile formula written out here; and the three refusals of the order checks.  No device.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "../../alphabeta_rs_amd/csrc/abn_tiles.hpp"

static uint64_t rng_state = 20261020ull;
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

int main() {
  size_t columns = 0, tiles = 0, empty = 0, whole_runs = 0, at_last = 0, neg_zero = 0, pairs = 0, fixed = 0;
  for (int it = 0; it < 60; ++it) {
    // the columns: n_runs runs of chromosomes drawn without repeat, in the order drawn
    const int n_runs = it == 0 ? 0 : 1 + (int)rnd(5);
    std::vector<int32_t> chrom;
    std::vector<uint32_t> start, end;
    std::vector<uint8_t> strand;
    std::vector<int> used;
    for (int r = 0; r < n_runs; ++r) {
      int c;
      do c = (int)rnd(4) == 0 ? 256 + (int)rnd(2) : (int)rnd(12);
      while (std::find(used.begin(), used.end(), c) != used.end());
      used.push_back(c);
      const long long len = rnd(4) == 0 ? 1 : 1 + rnd(300);
      const bool high = rnd(3) == 0;  // a run that ends at the highest start
      uint64_t pos = high ? 4294967295ull - 40ull * (uint64_t)len : rnd(1000);
      for (long long k = 0; k < len; ++k) {
        const bool pair = k > 0 && strand.back() == 0 && chrom.back() == c && rnd(8) == 0;  // the other strand, same start
        if (!pair) pos += 1 + rnd(39);
        if (high && k == len - 1 && !pair) pos = 4294967295ull;
        chrom.push_back(c), start.push_back((uint32_t)pos), end.push_back((uint32_t)pos), strand.push_back(pair ? 1 : 0);
        pairs += pair;
      }
      at_last += start.back() == 4294967295u;
    }
    const long long n_columns = (long long)chrom.size();
    columns += (size_t)n_columns;
    const auto xchrom = exact(chrom);
    const auto xstart = exact(start), xend = exact(end);
    const auto xstrand = exact(strand);
    const abn::CommonSites keys{xchrom.get(), xstart.get(), xend.get(), xstrand.get()};
    std::unique_ptr<long long[]> run_begin(new long long[abn::kCommonChroms]), run_end(new long long[abn::kCommonChroms]);
    std::vector<abn::TileRun> runs;
    abn::CommonRefusal refusal{0, -1, -1};
    if (!abn::tiles_runs_serial(keys, n_columns, run_begin.get(), run_end.get(), &runs, &refusal)) return fail("refused", it);
    if ((int)runs.size() != n_runs) return fail("the number of runs", it);
    long long at = 0;
    for (int r = 0; r < n_runs; ++r) {
      if (runs[(size_t)r].chromosome != used[(size_t)r] || runs[(size_t)r].first != at) return fail("a run's chromosome or begin", it);
      at += runs[(size_t)r].count;
      if (runs[(size_t)r].last_start != start[(size_t)at - 1]) return fail("a run's last start", it);
    }
    if (at != n_columns) return fail("the runs do not cover the columns", it);

    // the tiles
    std::vector<int32_t> tc;
    std::vector<long long> ts, te;
    for (int k = 0; k < 80; ++k) {
      const int kind = (int)rnd(8);
      int c = n_runs && kind != 0 ? used[rnd((uint32_t)n_runs)] : (int)rnd(258);
      long long a, b;
      if (n_columns && kind >= 3) {  // around two columns of the chromosome's run
        const abn::TileRun* run = nullptr;
        for (const auto& r : runs)
          if (r.chromosome == c) run = &r;
        const long long i = run->first + rnd((uint32_t)run->count), j = run->first + rnd((uint32_t)run->count);
        a = (long long)start[(size_t)std::min(i, j)] + (long long)rnd(3) - 1;
        b = (long long)start[(size_t)std::max(i, j)] + (long long)rnd(3);
        if (a < 0) a = 0;
        if (b > abn::kTilesPosEnd) b = abn::kTilesPosEnd;
        if (kind == 7) std::swap(a, b);
      } else if (kind == 1) {
        a = 0, b = abn::kTilesPosEnd;
        ++whole_runs;
      } else if (kind == 2) {
        a = b = rnd(2) ? abn::kTilesPosEnd : (long long)rnd(5000);
      } else {
        a = rnd(100000), b = a + rnd(100000);
      }
      if (!abn::tiles_interval_valid(c, a, b)) return fail("a valid interval is called invalid", it);
      tc.push_back(c), ts.push_back(a), te.push_back(b);
    }
    if (abn::tiles_interval_valid(258, 0, 1) || abn::tiles_interval_valid(-1, 0, 1) || abn::tiles_interval_valid(0, -1, 1) ||
        abn::tiles_interval_valid(0, 0, abn::kTilesPosEnd + 1))
      return fail("an invalid interval is called valid", it);
    const long long T = (long long)tc.size();
    const auto xtc = exact(tc);
    const auto xts = exact(ts), xte = exact(te);
    std::unique_ptr<long long[]> begin(new long long[(size_t)T]), endc(new long long[(size_t)T]);
    abn::tiles_search_serial(xstart.get(), run_begin.get(), run_end.get(), T, xtc.get(), xts.get(), xte.get(), begin.get(),
                             endc.get());
    for (long long t = 0; t < T; ++t) {  // the linear scan
      long long b = -1, e = -1, first = -1, last = -1;
      for (long long i = 0; i < n_columns; ++i) {
        if (chrom[(size_t)i] != tc[(size_t)t]) continue;
        if (first < 0) first = i;
        last = i + 1;
        if (b < 0 && (long long)start[(size_t)i] >= ts[(size_t)t]) b = i;
        if (e < 0 && (long long)start[(size_t)i] >= te[(size_t)t]) e = i;
      }
      if (first < 0) b = e = 0;
      else {
        if (b < 0) b = last;
        if (e < 0) e = last;
        if (te[(size_t)t] <= ts[(size_t)t]) e = b;
      }
      if (begin[(size_t)t] != b || endc[(size_t)t] != e) return fail("a tile's column range", it);
      empty += b == e;
    }
    tiles += (size_t)T;

    // the folds: n samples, merged bytes in rows of code_stride, levels in rows of n_columns
    const int n = 1 + (int)rnd(3);
    const long long code_stride = (n_columns + 15) / 16 * 16;
    std::vector<uint8_t> code((size_t)(n * code_stride), 0x7f);  // (the padding counts as counted: it must not be read)
    std::vector<double> level((size_t)(n * n_columns));
    for (int s = 0; s < n; ++s)
      for (long long i = 0; i < n_columns; ++i) {
        code[(size_t)(s * code_stride + i)] = (uint8_t)(rnd(3) | (rnd(3) ? abn::kCodeCounted : 0x80));
        level[(size_t)(s * n_columns + i)] = rnd(4) ? rnd(1000) / 1000.0 : -0.0;
      }
    const auto xcode = exact(code);
    const auto xlevel = exact(level);
    std::unique_ptr<double[]> sum(new double[(size_t)(n * T)]);
    std::unique_ptr<long long[]> kept(new long long[(size_t)(n * T)]);
    abn::tiles_fold_serial(xcode.get(), code_stride, xlevel.get(), n_columns, n, T, begin.get(), endc.get(), sum.get(),
                           kept.get());
    for (int s = 0; s < n; ++s)
      for (long long t = 0; t < T; ++t) {
        double want = 0.0;
        long long k = 0;
        for (long long i = begin[(size_t)t]; i < endc[(size_t)t]; ++i)
          if (code[(size_t)(s * code_stride + i)] & abn::kCodeCounted) {
            want += level[(size_t)(s * n_columns + i)];
            ++k;
            neg_zero += std::signbit(level[(size_t)(s * n_columns + i)]) ? 1 : 0;
          }
        if (kept[(size_t)(s * T + t)] != k || std::memcmp(&sum[(size_t)(s * T + t)], &want, 8) != 0) return fail("a tile's fold", it);
      }

    // the fixed tiles
    for (int rep = 0; rep < 3 && n_runs; ++rep) {
      const long long size = rep == 2 ? 3000000000LL : 1 + rnd(100000), step = rep == 0 ? 0 : 1 + rnd(200000);
      const long long F = abn::tiles_fixed_intervals(runs.data(), n_runs, size, step, nullptr, nullptr, nullptr);
      if (F <= 0 || F > 2000000) continue;
      std::unique_ptr<int32_t[]> fc(new int32_t[(size_t)F]);
      std::unique_ptr<long long[]> fs(new long long[(size_t)F]), fe(new long long[(size_t)F]);
      if (abn::tiles_fixed_intervals(runs.data(), n_runs, size, step, fc.get(), fs.get(), fe.get()) != F) return fail("F", it);
      long long t = 0;
      const long long st = step ? step : size;
      for (const auto& r : runs)
        for (long long k = 0; k * st <= (long long)r.last_start; ++k, ++t) {
          const long long want_end = k * st + size > abn::kTilesPosEnd ? abn::kTilesPosEnd : k * st + size;
          if (t >= F || fc[(size_t)t] != r.chromosome || fs[(size_t)t] != k * st || fe[(size_t)t] != want_end ||
              !abn::tiles_interval_valid(fc[(size_t)t], fs[(size_t)t], fe[(size_t)t]))
            return fail("a fixed tile", it);
        }
      if (t != F) return fail("the number of fixed tiles", it);
      fixed += (size_t)F;
    }
    if (abn::tiles_fixed_intervals(runs.data(), n_runs, 0, 0, nullptr, nullptr, nullptr) != -1 ||
        abn::tiles_fixed_intervals(runs.data(), n_runs, 5, -1, nullptr, nullptr, nullptr) != -1)
      return fail("size 0 or a negative step is taken", it);
  }
  // the refusals of the order checks
  {
    const std::vector<int32_t> chrom{2, 2, 1, 2}, bad{2, 300, 1, 1};
    const std::vector<uint32_t> asc{5, 9, 1, 20}, desc{5, 5, 1, 2};
    const std::vector<uint8_t> strand{0, 0, 0, 0};
    long long rb[abn::kCommonChroms], re[abn::kCommonChroms];
    std::vector<abn::TileRun> runs;
    abn::CommonRefusal r{0, -1, -1};
    if (abn::tiles_runs_serial(abn::CommonSites{chrom.data(), asc.data(), asc.data(), strand.data()}, 4, rb, re, &runs, &r) ||
        r.kind != abn::kCommonSplitRun + 1 || r.site != 3 || abn::common_refusal_text(r).find("split run") == std::string::npos)
      return fail("a split run is not refused", -1);
    const std::vector<int32_t> one{2, 2, 1, 1};
    if (abn::tiles_runs_serial(abn::CommonSites{one.data(), desc.data(), desc.data(), strand.data()}, 4, rb, re, &runs, &r) ||
        r.kind != abn::kCommonNotAscending + 1 || r.site != 1 ||
        abn::common_refusal_text(r).find("not ascending") == std::string::npos)
      return fail("a key that does not ascend is not refused", -1);
    if (abn::tiles_runs_serial(abn::CommonSites{bad.data(), asc.data(), asc.data(), strand.data()}, 4, rb, re, &runs, &r) ||
        r.kind != abn::kCommonBadKey + 1 || r.site != 1)
      return fail("a chromosome outside 0..257 is not refused", -1);
  }
  if (!columns || !tiles || !empty || !whole_runs || !at_last || !neg_zero || !pairs || !fixed) {
    std::printf("the cases miss a pattern: %zu %zu %zu %zu %zu %zu %zu %zu\n", columns, tiles, empty, whole_runs, at_last,
                neg_zero, pairs, fixed);
    return 1;
  }
  std::printf("tiles serial forms ok: %zu columns, %zu tiles (%zu empty), %zu fixed tiles, %zu runs up to 4294967295\n", columns,
              tiles, empty, fixed, at_last);
  return 0;
}
