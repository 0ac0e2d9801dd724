// The observation step (alphabeta_rs_amd/csrc/abn_sim.hpp) and the state census (abn_packed_census.hpp) in their host forms,
// built plain and with -fsanitize=address,undefined by tests/test_sim_study_cpu.py: every array a heap block of exactly its
// length.  The walk of the observation kernel's lane function — rows on y, workgroups of lanes grid-strided over a row's
// dwords, the low words drawn lazily or always, in place and into rows of a longer stride — against the law site by site;
// the walk of the census kernels' job structure — chunks of a window from its begin rounded down to 256 sites, a workgroup's
// lanes strided over a job's 16-byte loads, the edges masked, the partials summed per window — against the count field by
// field; the refusals one by one.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <memory>
#include <random>
#include <vector>

#include "../../alphabeta_rs_amd/csrc/abn_packed_census.hpp"
#include "../../alphabeta_rs_amd/csrc/abn_sim.hpp"

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

// rows of random fields 0..3 up to site L, 3 behind it, 0x5a between the rows
std::unique_ptr<uint8_t[]> random_rows(std::mt19937_64& rng, long long rows, long long L, long long stride) {
  std::unique_ptr<uint8_t[]> p(new uint8_t[(size_t)(rows * stride) + 1]);
  std::memset(p.get(), 0x5a, (size_t)(rows * stride) + 1);
  for (long long r = 0; r < rows; ++r) {
    std::memset(p.get() + r * stride, 0xff, (size_t)sim_row_bytes(L));
    for (long long k = 0; k < L; ++k) {
      const uint32_t f = (uint32_t)(rng() & 3);
      uint8_t& b = p[(size_t)(r * stride + (k >> 4) * 4 + (k & 3))];
      b = (uint8_t)(b ^ ((3u ^ f) << (2 * ((k >> 2) & 3))));
    }
  }
  return p;
}

int check_observe(std::mt19937_64& rng, long long rows, long long L, long long extra, int which) {
  const long long in_stride = sim_row_bytes(L), out_stride = sim_row_bytes(L) + extra;
  std::vector<int32_t> nodes_v;
  for (long long r = 0; r < rows; ++r) nodes_v.push_back((int32_t)((7 * r + 3) % kSimMaxNodes));
  std::vector<uint64_t> othr_v(9);
  for (int s = 0; s < 3; ++s) {
    uint64_t t[3] = {rng(), rng(), rng()};
    std::sort(t, t + 3);
    if (which % 3 == 1) t[0] = 0, t[2] = ~(uint64_t)0;
    if (which % 3 == 2) t[1] = t[0];
    std::copy(t, t + 3, othr_v.begin() + 3 * s);
  }
  const auto nodes = exact(nodes_v);
  const auto othr = exact(othr_v);
  const auto in = random_rows(rng, rows, L, in_stride);
  const size_t in_bytes = (size_t)(rows * in_stride), out_bytes = (size_t)(rows * out_stride);
  std::unique_ptr<uint8_t[]> in_exact(new uint8_t[in_bytes ? in_bytes : 1]);
  std::memcpy(in_exact.get(), in.get(), in_bytes);
  if (!sim_observe_refusal(rows, nodes.get(), othr.get(), L, in_exact.get(), in_stride, in_exact.get(), in_stride).empty())
    return fail("observe refused", which, L, rows);
  const uint64_t seed = 0x0123456789abcdefull + (uint64_t)which;
  std::unique_ptr<uint8_t[]> want(new uint8_t[out_bytes ? out_bytes : 1]), got(new uint8_t[out_bytes ? out_bytes : 1]);
  std::memset(want.get(), 0x5a, out_bytes);
  sim_observe_serial(seed, rows, nodes.get(), othr.get(), L, in_exact.get(), in_stride, want.get(), out_stride);
  for (long long r = 0; r < rows; ++r) {
    for (long long b = sim_row_bytes(L); b < out_stride; ++b)
      if (want[(size_t)(r * out_stride + b)] != 0x5a) return fail("the serial form wrote between the rows", which, L, r);
    for (long long k = 0; k < 4 * sim_row_bytes(L); ++k) {
      const size_t at = (size_t)((k >> 4) * 4 + (k & 3));
      const int shift = 2 * (int)((k >> 2) & 3);
      const uint32_t was = (in_exact[(size_t)(r * in_stride) + at] >> shift) & 3, is = (want[(size_t)(r * out_stride) + at] >> shift) & 3;
      if ((was == 3 || k >= L) && is != 3) return fail("a filtered field or one behind the last site is not 3", which, L, k);
    }
  }
  for (int lazy = 0; lazy < 2; ++lazy)
    for (long long blocks : {1ll, 3ll}) {
      std::memset(got.get(), 0x5a, out_bytes);
      if (lazy) sim_observe_walk<true>(seed, rows, nodes.get(), othr.get(), L, blocks, in_exact.get(), in_stride, got.get(), out_stride);
      else sim_observe_walk<false>(seed, rows, nodes.get(), othr.get(), L, blocks, in_exact.get(), in_stride, got.get(), out_stride);
      if (std::memcmp(want.get(), got.get(), out_bytes) != 0) return fail("the walk differs from the law", which, L, 10 * lazy + blocks);
    }
  // in place, the serial form and the walk: the bytes of the least stride
  for (int form = 0; form < 2; ++form) {
    std::unique_ptr<uint8_t[]> place(new uint8_t[in_bytes ? in_bytes : 1]);
    std::memcpy(place.get(), in_exact.get(), in_bytes);
    if (form == 0) sim_observe_serial(seed, rows, nodes.get(), othr.get(), L, place.get(), in_stride, place.get(), in_stride);
    else sim_observe_walk<true>(seed, rows, nodes.get(), othr.get(), L, 2, place.get(), in_stride, place.get(), in_stride);
    for (long long r = 0; r < rows; ++r)
      if (std::memcmp(place.get() + r * in_stride, want.get() + r * out_stride, (size_t)sim_row_bytes(L)) != 0)
        return fail("in place differs from out of place", which, L, form);
  }
  return 0;
}

int check_census(std::mt19937_64& rng, long long n, long long L, long long extra, long long chunk_sites) {
  const long long stride = sim_row_bytes(L) + extra;
  const auto packed_any = random_rows(rng, n, L, stride);
  const size_t bytes = (size_t)(n * stride);
  std::unique_ptr<uint8_t[]> packed(new uint8_t[bytes ? bytes : 1]);
  std::memcpy(packed.get(), packed_any.get(), bytes);
  std::vector<int64_t> cuts = {0, 1, 15, 16, 17, 255, 256, 257, 511, 512, 513, 1023, 1025, L};
  std::vector<int64_t> b_v, e_v;
  for (int64_t b : cuts)
    for (int64_t e : cuts)
      if (b <= e && e <= L) b_v.push_back(b), e_v.push_back(e);
  const int64_t W = (int64_t)b_v.size();
  const auto begin = exact(b_v);
  const auto end = exact(e_v);
  const auto chunk = exact(std::vector<long long>((size_t)W, chunk_sites));
  std::unique_ptr<uint64_t[]> want(new uint64_t[(size_t)(W * n * 3)]), got(new uint64_t[(size_t)(W * n * 3)]);
  if (!census_refusal(packed.get(), n, L, stride, begin.get(), end.get(), W, want.get()).empty()) return fail("census refused", n, L, W);
  census_windows_serial(packed.get(), n, stride, begin.get(), end.get(), W, want.get());
  census_windows_walk(packed.get(), n, stride, begin.get(), end.get(), W, chunk.get(), got.get());
  for (int64_t i = 0; i < W * n * 3; ++i)
    if (want[(size_t)i] != got[(size_t)i]) return fail("the census walk differs from the count", i / (n * 3), L, chunk_sites);
  return 0;
}

}  // namespace

int main() {
  std::mt19937_64 rng(20260101);
  const long long sizes[] = {0, 1, 15, 16, 17, 255, 256, 257, 1023, 1024, 1025, 4095, 4097, 3 * 16 * kSimThreads + 5};
  int which = 0;
  for (long long L : sizes)
    for (long long rows : {1ll, 8ll}) {
      if (check_observe(rng, rows, L, 0, which)) return 1;
      if (check_observe(rng, rows, L, 128, which + 1)) return 1;
      which += 2;
    }
  for (long long n : {1ll, 2ll, 5ll})
    for (long long L : {1025ll, 1300ll, 4097ll})
      for (long long chunk : {256ll, 512ll, (long long)kPmxWinPackedChunkSites}) {
        if (check_census(rng, n, L, n == 2 ? 64 : 0, chunk)) return 1;
        ++which;
      }
  // the observation's refusals, one by one
  {
    const int32_t nodes[2] = {0, 5}, far[2] = {0, 65535}, negative[2] = {-1, 0};
    uint64_t othr[9] = {1, 2, 3, 0, 0, ~(uint64_t)0, 5, 5, 5}, bad[9] = {1, 2, 3, 4, 3, 9, 5, 5, 5};
    std::unique_ptr<uint8_t[]> a(new uint8_t[256]), b(new uint8_t[256]);
    auto r = [&](int64_t rows, const int32_t* nd, const uint64_t* t, int64_t L, const void* in, int64_t is, const void* out, int64_t os) {
      return sim_observe_refusal(rows, nd, t, L, in, is, out, os);
    };
    if (!r(2, nodes, othr, 100, a.get(), 64, b.get(), 128).empty() || !r(2, nodes, othr, 100, a.get(), 64, a.get(), 64).empty() ||
        !r(2, nodes, othr, 0, a.get(), 0, a.get(), 64).empty())
      return fail("valid arguments refused", 0, 0, 0);
    if (r(0, nodes, othr, 100, a.get(), 64, b.get(), 64).empty() || r(65536, nodes, othr, 100, a.get(), 64, b.get(), 64).empty() ||
        r(2, far, othr, 100, a.get(), 64, b.get(), 64).empty() || r(2, negative, othr, 100, a.get(), 64, b.get(), 64).empty() ||
        r(2, nodes, bad, 100, a.get(), 64, b.get(), 64).empty() || r(2, nodes, othr, -1, a.get(), 64, b.get(), 64).empty() ||
        r(2, nodes, othr, kSimMaxSites + 1, a.get(), (kSimMaxSites + 256) / 4, b.get(), (kSimMaxSites + 256) / 4).empty() ||
        r(2, nodes, othr, 100, a.get(), 96, b.get(), 64).empty() || r(2, nodes, othr, 257, a.get(), 128, b.get(), 64).empty() ||
        r(2, nodes, othr, 100, a.get(), 64, a.get(), 128).empty() || r(2, nodes, othr, 100, a.get(), 64, a.get() + 64, 64).empty() ||
        r(2, nullptr, othr, 100, a.get(), 64, b.get(), 64).empty() || r(2, nodes, nullptr, 100, a.get(), 64, b.get(), 64).empty() ||
        r(2, nodes, othr, 100, nullptr, 64, b.get(), 64).empty() || r(2, nodes, othr, 100, a.get(), 64, nullptr, 64).empty())
      return fail("an invalid argument was taken", 0, 0, 0);
    double miscall[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, dropout[3] = {0, 0.5, 1}, off[9] = {1, 1e-9, 0, 0, 1, 0, 0, 0, 1};
    uint64_t t[9];
    if (!sim_obs_thresholds(miscall, dropout, t).empty() || t[0] != ~(uint64_t)0 || t[3] != 0 || t[4] != (uint64_t)1 << 63 ||
        t[5] != (uint64_t)1 << 63 || t[6] != 0 || t[8] != 0)
      return fail("the identity's thresholds", (long long)t[3], (long long)t[4], (long long)t[8]);
    if (sim_obs_thresholds(off, dropout, t).empty() || sim_obs_thresholds(nullptr, dropout, t).empty()) return fail("thresholds taken", 0, 0, 0);
  }
  std::printf("sim study ok: %d cases\n", which);
  return 0;
}
