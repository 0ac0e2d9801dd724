// The simulated methylomes (alphabeta_rs_amd/csrc/abn_sim.hpp) in their serial forms, built plain and with
// -fsanitize=address,undefined by tests/test_sim_cpu.py: every array a heap block of exactly its length.  The walk of the
// kernel's structure — workgroups of lanes grid-strided over a row's dwords, a lane's trip the nodes in index order, the
// parent's dword from the lane's register or from the row the lane wrote, unemitted live nodes in scratch rows, the edge
// dword masked, the low words drawn lazily or always — against the law site by site, over the sizes around the dword, the
// 64-byte step, a wavefront and a workgroup, over chains, stars, unemitted internal nodes and founders and dead leaves,
// under thresholds from rates and thresholds over the whole 64-bit range, into rows of the least stride and of a longer one.
#include <cstdio>
#include <cstring>
#include <memory>
#include <random>
#include <vector>

#include "../../alphabeta_rs_amd/csrc/abn_sim.hpp"

using namespace abn;

namespace {

int fail(const char* what, long long a, long long b, long long c) {
  std::printf("FAILED: %s (%lld, %lld, %lld)\n", what, a, b, c);
  return 1;
}

struct Tree {
  std::vector<int32_t> parent, generation;
  std::vector<uint8_t> emit;
};

template <class T>
std::unique_ptr<T[]> exact(const std::vector<T>& v) {  // a heap block of exactly v.size() entries
  std::unique_ptr<T[]> p(new T[v.size()]);
  std::copy(v.begin(), v.end(), p.get());
  return p;
}

int check(const Tree& t, const std::vector<uint64_t>& thr_v, long long L, long long extra_stride, int which) {
  const int32_t V = (int32_t)t.parent.size();
  const auto parent = exact(t.parent);
  const auto emit = exact(t.emit);
  const auto thr = exact(thr_v);
  const long long stride = sim_row_bytes(L) + extra_stride;
  if (!sim_refusal(V, parent.get(), thr.get(), emit.get(), L, parent.get(), stride).empty()) return fail("refused", which, L, V);
  const SimPlan plan = sim_plan(V, parent.get(), emit.get());
  const auto nodes = exact(plan.nodes);
  const size_t bytes = (size_t)plan.n_emit * (size_t)stride;
  std::unique_ptr<uint8_t[]> want(new uint8_t[bytes]), got(new uint8_t[bytes]);
  std::memset(want.get(), 0x5a, bytes);
  sim_codes_serial(0x0123456789abcdefull + (uint64_t)which, V, parent.get(), thr.get(), emit.get(), L, want.get(), stride);
  for (long long r = 0; r < plan.n_emit; ++r) {
    for (long long b = sim_row_bytes(L); b < stride; ++b)
      if (want[(size_t)(r * stride + b)] != 0x5a) return fail("the serial form wrote between the rows", which, L, r);
    for (long long k = L; k < 4 * sim_row_bytes(L); ++k)
      if (((want[(size_t)(r * stride + (k >> 4) * 4 + (k & 3))] >> (2 * ((k >> 2) & 3))) & 3) != 3)
        return fail("a field behind the last site is not 3", which, L, k);
  }
  const size_t scratch_bytes = (size_t)plan.n_scratch * (size_t)sim_row_bytes(L);
  for (int lazy = 0; lazy < 2; ++lazy)
    for (long long blocks : {1ll, 3ll}) {
      std::unique_ptr<uint8_t[]> scratch(scratch_bytes ? new uint8_t[scratch_bytes] : nullptr);
      std::memset(got.get(), 0x5a, bytes);
      if (lazy) sim_codes_walk<true>(0x0123456789abcdefull + (uint64_t)which, V, nodes.get(), thr.get(), L, blocks, got.get(), stride, scratch.get());
      else sim_codes_walk<false>(0x0123456789abcdefull + (uint64_t)which, V, nodes.get(), thr.get(), L, blocks, got.get(), stride, scratch.get());
      if (std::memcmp(want.get(), got.get(), bytes) != 0) return fail("the walk differs from the law", which, L, 10 * lazy + blocks);
    }
  return 0;
}

}  // namespace

int main() {
  const std::vector<Tree> trees = {
      {{-1}, {3}, {1}},
      {{-1, 0, 1, 2}, {0, 1, 3, 4}, {1, 1, 1, 1}},
      {{-1, 0, 0, 0, 0}, {1, 2, 2, 5, 9}, {1, 1, 1, 1, 1}},
      {{-1, 0, 0, 1, 1, 2, 2, 3}, {2, 3, 3, 5, 8, 4, 9, 5}, {1, 1, 1, 1, 1, 1, 1, 1}},
      {{-1, 0, 0, 1, 1, 2, 2, 3}, {2, 3, 3, 5, 8, 4, 9, 5}, {1, 0, 0, 0, 1, 1, 1, 1}},
      {{-1, 0, 0, 1, 1, 2, 2, 3, 4}, {0, 3, 3, 5, 8, 4, 9, 5, 9}, {0, 0, 1, 0, 1, 1, 0, 1, 0}},
      {{-1, 0, 1, 1, 0}, {2, 2, 2, 4, 2}, {1, 1, 0, 1, 1}},
  };
  const long long sizes[] = {0, 1, 15, 16, 17, 255, 256, 257, 1023, 1024, 1025, 4095, 4097, 3 * 16 * kSimThreads + 5};
  std::mt19937_64 rng(20260101);
  int which = 0;
  for (const Tree& t : trees) {
    const int32_t V = (int32_t)t.parent.size();
    std::vector<uint64_t> rates((size_t)V * 6), any((size_t)V * 6);
    const auto parent = exact(t.parent);
    const auto generation = exact(t.generation);
    std::unique_ptr<uint64_t[]> thr(new uint64_t[(size_t)V * 6]);
    if (!sim_thresholds(0.1, 0.2, 0.7, 0.3, V, parent.get(), generation.get(), thr.get()).empty()) return fail("thresholds refused", which, V, 0);
    std::copy(thr.get(), thr.get() + (size_t)V * 6, rates.begin());
    for (size_t i = 0; i < any.size(); i += 2) {
      const uint64_t a = rng(), b = rng();
      any[i] = a < b ? a : b, any[i + 1] = a < b ? b : a;
    }
    any[0] = 0, any[1] = ~(uint64_t)0;  // and the two ends of the range
    for (long long L : sizes) {
      if (check(t, rates, L, 0, which)) return 1;
      if (check(t, any, L, 128, which)) return 1;
      ++which;
    }
  }
  // the law's refusals, one by one
  {
    const int32_t parent[3] = {-1, 0, 1}, bad_parent[3] = {-1, 1, 0}, rooted[3] = {0, 0, 1};
    const uint8_t emit[3] = {1, 0, 1}, none[3] = {0, 0, 0};
    uint64_t thr[18], bad_thr[18];
    for (int i = 0; i < 18; ++i) thr[i] = bad_thr[i] = (uint64_t)(i % 2) << 63;
    bad_thr[8] = 5, bad_thr[9] = 4;
    uint8_t out[64];
    if (!sim_refusal(3, parent, thr, emit, 100, out, 64).empty()) return fail("valid arguments refused", 0, 0, 0);
    if (sim_refusal(0, parent, thr, emit, 100, out, 64).empty() || sim_refusal(kSimMaxNodes + 1, parent, thr, emit, 100, out, 64).empty() ||
        sim_refusal(3, bad_parent, thr, emit, 100, out, 64).empty() || sim_refusal(3, rooted, thr, emit, 100, out, 64).empty() ||
        sim_refusal(3, parent, bad_thr, emit, 100, out, 64).empty() || sim_refusal(3, parent, thr, none, 100, out, 64).empty() ||
        sim_refusal(3, parent, thr, emit, -1, out, 64).empty() || sim_refusal(3, parent, thr, emit, kSimMaxSites + 1, out, (kSimMaxSites + 256) / 4).empty() ||
        sim_refusal(3, parent, thr, emit, 257, out, 64).empty() || sim_refusal(3, parent, thr, emit, 100, out, 96).empty() ||
        sim_refusal(3, nullptr, thr, emit, 100, out, 64).empty() || sim_refusal(3, parent, nullptr, emit, 100, out, 64).empty() ||
        sim_refusal(3, parent, thr, nullptr, 100, out, 64).empty() || sim_refusal(3, parent, thr, emit, 100, nullptr, 64).empty())
      return fail("an invalid argument was taken", 0, 0, 0);
  }
  std::printf("sim ok: %d cases\n", 4 * which);
  return 0;
}
