// Stand-alone driver for the serial forms of the block bootstrap (alphabeta_rs_amd/csrc/abn_blocks.hpp), built by
// tests/test_blocks_cpu.py plain and with AddressSanitizer + UndefinedBehaviorSanitizer and run directly.  The shapes of the
// CPU and GPU tests — rows 1, 16, 17; blocks 1, 63, 64, 65, 129 in a group that begins off a multiple of 64; pairs 1, 3, 45;
// three groups of which one holds a single block and one is empty; the accumulator-flush shape; the counts on both sides of
// the histogram threshold — through block_shape_refusal, block_tables_refusal, block_counts_refusal, block_resample_host and
// block_counts_host, every array in a heap block of exactly its length (a read or write past either end is a report), the
// sums against a column-by-column loop and the counts against their row sums.  No device.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "../../alphabeta_rs_amd/csrc/abn_blocks.hpp"

static uint64_t rng_state = 20261020ull;
static uint64_t rnd() {
  rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
  return rng_state >> 20;
}

template <class T>
static std::unique_ptr<T[]> block(size_t n) {  // a heap block of exactly n elements
  return std::unique_ptr<T[]>(new T[n]);
}

static int fail(const char* what, const char* name) {
  std::printf("%s: %s\n", name, what);
  return 1;
}

static int resample_case(const char* name, std::vector<int64_t> gb, std::vector<int64_t> ge, long long rows, long long T,
                         long long P, long long n, bool all_largest) {
  const long long G = (long long)gb.size();
  const uint64_t values[6] = {0, 127, 128, (1ull << 14) - 1, 1ull << 14, (1ull << 35) - 1};
  auto g_begin = block<int64_t>((size_t)G), g_end = block<int64_t>((size_t)G);
  for (long long g = 0; g < G; ++g) g_begin[g] = gb[(size_t)g], g_end[g] = ge[(size_t)g];
  auto counts = block<uint8_t>((size_t)(G * rows * T));
  auto both = block<uint64_t>((size_t)(T * P)), diff = block<uint64_t>((size_t)(T * P));
  auto level = block<double>((size_t)(n * T));
  auto kept = block<int64_t>((size_t)(n * T));
  for (long long i = 0; i < G * rows * T; ++i) counts[i] = all_largest ? 127 : (rnd() % 10 == 0 ? 127 : (uint8_t)(rnd() % 4));
  for (long long i = 0; i < T * P; ++i) both[i] = all_largest ? values[5] : values[rnd() % 6], diff[i] = all_largest ? values[5] : values[rnd() % 6];
  for (long long i = 0; i < n * T; ++i) level[i] = (double)(rnd() % 100000) / 7.0, kept[i] = (int64_t)(rnd() % (1 << 20));
  uint64_t largest = 0;
  if (!abn::block_shape_refusal(G, g_begin.get(), g_end.get(), rows, T).empty()) return fail("shape refused", name);
  if (!abn::block_tables_refusal(T, P, n, both.get(), diff.get(), level.get(), kept.get(), &largest).empty())
    return fail("tables refused", name);
  if (!abn::block_counts_refusal(G, g_begin.get(), g_end.get(), rows, T, counts.get()).empty()) return fail("counts refused", name);
  if (abn::block_digits_of(largest) < 1 || abn::block_digits_of(largest) > abn::kBlockDigitsMax) return fail("digits", name);
  auto ob = block<uint64_t>((size_t)(G * rows * P)), od = block<uint64_t>((size_t)(G * rows * P));
  auto ov = block<double>((size_t)(G * rows * P)), ol = block<double>((size_t)(G * rows * n));
  auto ok = block<int64_t>((size_t)(G * rows * n));
  abn::block_resample_host(G, g_begin.get(), g_end.get(), rows, counts.get(), T, P, n, both.get(), diff.get(), level.get(),
                           kept.get(), ob.get(), od.get(), ov.get(), ol.get(), ok.get());
  for (long long g = 0; g < G; ++g)
    for (long long r = 0; r < rows; ++r) {
      const uint8_t* c = counts.get() + (g * rows + r) * T;
      for (long long p = 0; p < P; ++p) {
        uint64_t sb = 0, sd = 0;  // the digits recombined: sum_d 2^(7 d) sum_t c digit_d
        for (int d = 0; d < abn::kBlockDigitsMax; ++d) {
          uint64_t pb = 0, pd = 0;
          for (long long t = gb[(size_t)g]; t < ge[(size_t)g]; ++t)
            pb += (uint64_t)c[t] * abn::block_digit(both[t * P + p], d), pd += (uint64_t)c[t] * abn::block_digit(diff[t * P + p], d);
          sb += pb << (abn::kBlockDigitBits * d), sd += pd << (abn::kBlockDigitBits * d);
        }
        const size_t at = (size_t)((g * rows + r) * P + p);
        if (ob[at] != sb || od[at] != sd) return fail("a sum differs from its digits' sums", name);
        const double want = (double)sd / (2.0 * (double)sb);
        if (std::memcmp(&want, &ov[at], 8) != 0 && !(std::isnan(want) && std::isnan(ov[at]))) return fail("dvalue", name);
        if (gb[(size_t)g] == ge[(size_t)g] && (sb != 0 || !std::isnan(ov[at]))) return fail("an empty group", name);
      }
      for (long long s = 0; s < n; ++s) {
        int64_t k = 0;
        for (long long t = gb[(size_t)g]; t < ge[(size_t)g]; ++t) k += (int64_t)c[t] * kept[s * T + t];
        if (ok[(size_t)((g * rows + r) * n + s)] != k) return fail("kept", name);
        if (!(ol[(size_t)((g * rows + r) * n + s)] >= 0.0)) return fail("level", name);
      }
    }
  // any output may be null
  abn::block_resample_host(G, g_begin.get(), g_end.get(), rows, counts.get(), T, P, n, both.get(), diff.get(), level.get(),
                           kept.get(), nullptr, nullptr, ov.get(), nullptr, nullptr);
  abn::block_resample_host(G, g_begin.get(), g_end.get(), rows, counts.get(), T, P, n, both.get(), diff.get(), level.get(),
                           kept.get(), nullptr, nullptr, nullptr, ol.get(), nullptr);
  // the refusals leave the arrays alone
  if (T * P > 0) {
    both[T * P - 1] = 1ull << 35;
    if (abn::block_tables_refusal(T, P, n, both.get(), diff.get(), level.get(), kept.get(), nullptr).empty())
      return fail("2^35 taken", name);
  }
  if (ge[0] > gb[0]) {
    counts[gb[0]] = 128;
    if (abn::block_counts_refusal(G, g_begin.get(), g_end.get(), rows, T, counts.get()).empty()) return fail("128 taken", name);
  }
  return 0;
}

static int counts_case(long long hist) {
  const long long sizes[8] = {1, 3, 4, 5, 257, hist - 1, hist, hist + 1};
  const long long G = 8, R = 2;
  auto gid = block<uint32_t>(8);
  auto gb = block<int64_t>(8), ge = block<int64_t>(8);
  long long at = 2;
  for (int g = 0; g < 8; ++g) gid[g] = g == 7 ? 0xffffffffu : (uint32_t)(3 * g), gb[g] = at, ge[g] = at + sizes[g], at += sizes[g] + 1;
  const long long T = at + 2;
  if (!abn::block_shape_refusal(G, gb.get(), ge.get(), R + 1, T).empty()) return fail("shape refused", "counts");
  auto counts = block<uint8_t>((size_t)(G * (R + 1) * T));
  if (!abn::block_counts_host(20260101ull, G, gid.get(), gb.get(), ge.get(), R, T, counts.get())) return fail("a count above 127", "counts");
  for (long long g = 0; g < G; ++g)
    for (long long r = 0; r <= R; ++r) {
      long long inside = 0, outside = 0;
      for (long long t = 0; t < T; ++t) (t >= gb[g] && t < ge[g] ? inside : outside) += counts[(g * (R + 1) + r) * T + t];
      if (inside != sizes[g] || outside != 0) return fail("a row does not hold T_g draws", "counts");
    }
  const int64_t bad_b[2] = {0, 2}, bad_e[2] = {3, 4};
  if (abn::block_shape_refusal(2, bad_b, bad_e, 1, 4).empty()) return fail("overlapping groups taken", "counts");
  if (abn::block_shape_refusal(1, bad_b, bad_e, abn::kBlockReplicatesMax + 2, 4).empty()) return fail("2^20 - 1 replicates taken", "counts");
  return 0;
}

int main() {
  const long long row_counts[3] = {1, 16, 17}, blocks[5] = {1, 63, 64, 65, 129}, pairs[3] = {1, 3, 45};
  for (long long rows : row_counts)
    for (long long b : blocks)
      for (long long p : pairs)
        if (resample_case("one group", {3}, {3 + b}, rows, b + 7, p, 2, false)) return 1;
  if (resample_case("three groups", {5, 70, 77}, {6, 70, 227}, 17, 300, 45, 4, false)) return 1;
  if (resample_case("three groups, one pair", {63, 64, 130}, {64, 64, 257}, 1, 257, 1, 1, false)) return 1;
  if (resample_case("no pair, no sample", {0}, {9}, 2, 9, 0, 0, false)) return 1;
  if (resample_case("the flush", {0}, {abn::kBlockFlush + 65}, 1, abn::kBlockFlush + 65, 1, 1, true)) return 1;
  if (counts_case(abn::kBlockHist)) return 1;
  std::printf("block bootstrap serial forms ok\n");
  return 0;
}
