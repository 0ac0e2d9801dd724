// Region states (alphabeta_rs_amd/csrc/abn_regions.hpp) in their host forms, built plain and with
// -fsanitize=address,undefined by tests/test_regions_cpu.py: every array a heap block of exactly its length.  The walk of
// the kernel's structure — a workgroup of 256 lanes per 64-byte super-step of an output row, a lane per output field walking
// its window's dwords with the edges masked, 16 lanes ORing one dword, the long windows through the census's walk — against
// the law field by field, with long_sites at the default and at 64; the rule on planted counts; the refusals one by one.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <memory>
#include <random>
#include <vector>

#include "../../alphabeta_rs_amd/csrc/abn_regions.hpp"

using namespace abn;

namespace {

int fail(const char* what, long long a, long long b, long long c) {
  std::printf("FAILED: %s (%lld, %lld, %lld)\n", what, a, b, c);
  return 1;
}

template <class T>
std::unique_ptr<T[]> exact(const std::vector<T>& v) {  // a heap block of exactly v.size() entries
  std::unique_ptr<T[]> p(new T[v.size() ? v.size() : 1]);
  std::copy(v.begin(), v.end(), p.get());
  return p;
}

long long stride_of(long long sites) { return sites <= 0 ? 0 : (sites + 255) / 256 * 64; }

// n rows of exactly stride_of(L) bytes: random fields 0..3 up to site L, 3 behind it
std::unique_ptr<uint8_t[]> random_rows(std::mt19937_64& rng, long long rows, long long L) {
  const long long stride = stride_of(L);
  std::unique_ptr<uint8_t[]> p(new uint8_t[(size_t)(rows * stride)]);  // (L >= 1 here)
  std::memset(p.get(), 0xff, (size_t)(rows * stride));
  for (long long r = 0; r < rows; ++r)
    for (long long k = 0; k < L; ++k) {
      const uint32_t f = (uint32_t)(rng() & 3);
      uint8_t& b = p[(size_t)(r * stride + (k >> 4) * 4 + (k & 3))];
      b = (uint8_t)(b ^ ((3u ^ f) << (2 * ((k >> 2) & 3))));
    }
  return p;
}

int check_states(std::mt19937_64& rng, long long n, long long L, int src_kind, const RegionRule rule, long long long_sites) {
  const long long stride = stride_of(L);
  const std::unique_ptr<uint8_t[]> packed = random_rows(rng, n, L);
  std::vector<int64_t> bv, ev;
  const long long cuts[] = {0, 1, 15, 16, 17, 63, 64, 65, 255, 256, 257, L};
  for (long long a : cuts)
    for (long long b : cuts)
      if (a <= b && b <= L) bv.push_back(a), ev.push_back(b);
  for (int k = 0; k < 40; ++k) {  // short tiles one behind the other, then random ranges
    const long long a = L ? (long long)(rng() % (uint64_t)(L + 1)) : 0, len = (long long)(rng() % 41);
    bv.push_back(a), ev.push_back(std::min(L, a + len));
  }
  const long long T = (long long)bv.size();
  std::vector<int32_t> sv;
  if (src_kind == 1) {  // a permutation
    for (long long t = 0; t < T; ++t) sv.push_back((int32_t)t);
    std::shuffle(sv.begin(), sv.end(), rng);
  } else if (src_kind == 2) {  // repeats and omissions, C = 257
    for (int c = 0; c < 257; ++c) sv.push_back((int32_t)(rng() % (uint64_t)T));
  }
  const long long C = src_kind ? (long long)sv.size() : T, out_stride = stride_of(C);
  const std::unique_ptr<int64_t[]> begin = exact(bv), end = exact(ev);
  const std::unique_ptr<int32_t[]> src = exact(sv);
  const int32_t* sp = src_kind ? src.get() : nullptr;
  std::unique_ptr<uint8_t[]> want(new uint8_t[(size_t)(n * out_stride)]), got(new uint8_t[(size_t)(n * out_stride)]);
  std::memset(want.get(), 0x5a, (size_t)(n * out_stride));
  std::memset(got.get(), 0xa5, (size_t)(n * out_stride));
  const std::string why = region_refusal(packed.get(), n, L, stride, begin.get(), end.get(), T, sp, C, (int64_t)rule.lo_num,
                                         (int64_t)rule.hi_num, (int64_t)rule.den, (int64_t)rule.min_kept, long_sites, want.get());
  if (!why.empty()) return fail(why.c_str(), n, L, src_kind);
  region_states_serial(packed.get(), n, stride, begin.get(), end.get(), sp, C, rule, want.get(), out_stride);
  region_states_walk(packed.get(), n, stride, begin.get(), end.get(), T, sp, C, rule, region_long_sites(long_sites), got.get(),
                     out_stride);
  if (std::memcmp(want.get(), got.get(), (size_t)(n * out_stride)) != 0) return fail("the walk differs from the law", n, L, long_sites);
  // the padding: every field from C to the end of the stride is 3
  for (long long s = 0; s < n; ++s)
    for (long long c = C; c < out_stride * 4; ++c)
      if (((want[(size_t)(s * out_stride + (c >> 4) * 4 + (c & 3))] >> (2 * ((c >> 2) & 3))) & 3) != 3)
        return fail("a padding field is not 3", s, c, C);
  return 0;
}

int check_call() {
  const RegionRule r{1, 2, 3, 2};
  // kept below min_kept; m den against lo 2 kept = 2 kept and hi 2 kept = 4 kept
  if (region_call(1, 0, 0, r) != 3 || region_call(0, 0, 0, r) != 3) return fail("kept < min_kept", 0, 0, 0);
  if (region_call(1, 2, 0, r) != 1 || region_call(0, 2, 1, r) != 1) return fail("equality on either side is 1", 0, 0, 0);
  if (region_call(2, 1, 0, r) != 0 || region_call(0, 1, 2, r) != 2) return fail("one unit beyond either threshold", 0, 0, 0);
  const RegionRule q{1, 3, 4, 1};
  if (region_call(1, 0, 0, q) != 0 || region_call(0, 1, 0, q) != 1 || region_call(0, 0, 1, q) != 2) return fail("identity rule", 0, 0, 0);
  const uint64_t big = 1ull << 34;
  const RegionRule w{1u << 19, 1u << 19, 1u << 20, 1};  // lo = hi = 1/2
  if (region_call(big / 2, 0, big / 2, w) != 1) return fail("2^34 sites at the threshold", 0, 0, 0);
  if (region_call(big / 2, 1, big / 2 - 1, w) != 0 || region_call(big / 2 - 1, 1, big / 2, w) != 2) return fail("one unit off", 0, 0, 0);
  return 0;
}

int check_refusals() {
  std::mt19937_64 rng(3);
  const std::unique_ptr<uint8_t[]> packed = random_rows(rng, 1, 300);
  const int64_t b[2] = {0, 10}, e[2] = {5, 300};
  const int32_t s_ok[3] = {1, 0, 1}, s_bad[3] = {0, 2, 1};
  uint8_t out[64];
  const auto r = [&](int64_t T, const int32_t* src, int64_t C, int64_t lo, int64_t hi, int64_t den, int64_t mk, int64_t ls) {
    return region_refusal(packed.get(), 1, 300, 128, b, e, T, src, C, lo, hi, den, mk, ls, out);
  };
  if (!r(2, s_ok, 3, 1, 2, 3, 1, 0).empty() || !r(2, nullptr, 2, 0, 4, 4, 1, 64).empty()) return fail("refused what is valid", 0, 0, 0);
  if (r(2, s_bad, 3, 1, 2, 3, 1, 0).find("column 1") == std::string::npos) return fail("src outside", 0, 0, 0);
  if (r(2, nullptr, 3, 1, 2, 3, 1, 0).empty() || r(2, s_ok, 3, 2, 1, 3, 1, 0).empty() || r(2, s_ok, 3, 1, 4, 3, 1, 0).empty() ||
      r(2, s_ok, 3, 1, 2, (1 << 20) + 1, 1, 0).empty() || r(2, s_ok, 3, 1, 2, 0, 1, 0).empty() || r(2, s_ok, 3, 1, 2, 3, 0, 0).empty() ||
      r(2, s_ok, 3, 1, 2, 3, 1, -16).empty() || r(2, s_ok, 3, 1, 2, 3, 1, 40).empty() || r(1ll << 31, s_ok, 3, 1, 2, 3, 1, 0).empty() ||
      r(2, s_ok, 1ll << 31, 1, 2, 3, 1, 0).empty() || r(2, s_ok, -1, 1, 2, 3, 1, 0).empty())
    return fail("took what is refused", 0, 0, 0);
  const int64_t e_bad[2] = {5, 301};
  if (region_refusal(packed.get(), 1, 300, 128, b, e_bad, 2, nullptr, 2, 1, 2, 3, 1, 0, out).find("window 1") == std::string::npos)
    return fail("a window outside the rows", 0, 0, 0);
  return 0;
}

}  // namespace

int main() {
  std::mt19937_64 rng(20260101);
  const RegionRule rules[] = {{1, 2, 3, 1}, {0, 7, 7, 2}, {5, 5, 9, 5}, {1u << 18, 3u << 18, 1u << 20, 1}};
  const long long Ls[] = {1, 15, 16, 17, 255, 256, 257, 4097, 9000};
  int which = 0;
  for (long long L : Ls)
    for (long long n : {1ll, 3ll})
      for (int src_kind = 0; src_kind < 3; ++src_kind)
        for (long long long_sites : {0ll, 64ll}) {
          if (check_states(rng, n, L, src_kind, rules[which % 4], long_sites)) return 1;
          ++which;
        }
  if (check_call()) return 1;
  if (check_refusals()) return 1;
  std::printf("regions ok: %d shapes\n", which);
  return 0;
}
