// Stand-alone driver for the common-site step (alphabeta_rs_amd/csrc/abn_sites_common.hpp), built by
// tests/test_sites_common_cpu.py with AddressSanitizer + UndefinedBehaviorSanitizer and run directly.  Seeded cases of 1 to
// 5 samples — empty samples, a sample of one site beside one of 3000, chromosomes missing from a sample, the runs in the
// order 1, 10, 2, 256, 257, every site common, none common, common counts on both sides of 64 and 256 — through
// sites_common_serial, every input and output array in a heap block of exactly its length (a read or write past either end
// is a report), against an intersection by counting keys in a std::map written out here; and samples with a split run, a
// descending neighbour, a duplicate key and the runs in another order, which must be refused at the expected site.  No
// device.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <tuple>
#include <vector>

#include "../../alphabeta_rs_amd/csrc/abn_sites_common.hpp"

using Key = std::tuple<int32_t, uint32_t, uint32_t, uint32_t>;  // chromosome, start, end, strand
using Sample = std::vector<Key>;

static uint64_t rng_state = 20261019ull;
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

static int failures = 0;
#define CHECK(cond, ...)                 \
  do {                                   \
    if (!(cond)) {                       \
      std::printf("FAILED: " __VA_ARGS__); \
      std::printf("\n");                 \
      ++failures;                        \
    }                                    \
  } while (0)

struct Result {
  long long n_common;
  abn::CommonRefusal refusal;
  std::vector<uint8_t> keep;
};

static Result run(const std::vector<Sample>& samples) {
  const int n = (int)samples.size();
  std::vector<long long> off((size_t)n + 1, 0);
  std::vector<int32_t> chrom;
  std::vector<uint32_t> start, end;
  std::vector<uint8_t> strand;
  for (int s = 0; s < n; ++s) {
    off[(size_t)s + 1] = off[(size_t)s] + (long long)samples[(size_t)s].size();
    for (const Key& k : samples[(size_t)s]) {
      chrom.push_back(std::get<0>(k));
      start.push_back(std::get<1>(k));
      end.push_back(std::get<2>(k));
      strand.push_back((uint8_t)std::get<3>(k));
    }
  }
  const auto poff = exact(off);
  const auto pchrom = exact(chrom);
  const auto pstart = exact(start);
  const auto pend = exact(end);
  const auto pstrand = exact(strand);
  std::unique_ptr<uint8_t[]> keep(new uint8_t[chrom.size()]);
  std::memset(keep.get(), 7, chrom.size());
  Result r;
  r.n_common = abn::sites_common_serial(abn::CommonSites{pchrom.get(), pstart.get(), pend.get(), pstrand.get()}, n,
                                        poff.get(), keep.get(), &r.refusal);
  r.keep.assign(keep.get(), keep.get() + chrom.size());
  return r;
}

// the samples' keys ordered as the files are: the chromosomes in chrom_order, (start, end, strand) ascending inside
static void order(Sample& s, const std::vector<int32_t>& chrom_order) {
  auto rank = [&](int32_t c) { return std::find(chrom_order.begin(), chrom_order.end(), c) - chrom_order.begin(); };
  std::sort(s.begin(), s.end(), [&](const Key& a, const Key& b) {
    if (std::get<0>(a) != std::get<0>(b)) return rank(std::get<0>(a)) < rank(std::get<0>(b));
    return std::tie(std::get<1>(a), std::get<2>(a), std::get<3>(a)) < std::tie(std::get<1>(b), std::get<2>(b), std::get<3>(b));
  });
}

// n_common keys in every sample, n_extra keys in some and not in all (none for one sample)
static std::vector<Sample> make(int n, int n_common, int n_extra, const std::vector<int32_t>& chrom_order) {
  std::map<Key, int> all;
  const uint32_t span = (uint32_t)std::max(8, (n_common + n_extra) / 4);
  const size_t want = (size_t)n_common + (n > 1 ? (size_t)n_extra : 0);
  while (all.size() < want) {
    const uint32_t s = 1 + rnd(span);
    all[Key{chrom_order[rnd((uint32_t)chrom_order.size())], s, s + rnd(3), rnd(3)}] = 0;
  }
  std::vector<Key> keys;
  for (const auto& kv : all) keys.push_back(kv.first);
  for (size_t i = keys.size(); i > 1; --i) std::swap(keys[i - 1], keys[rnd((uint32_t)i)]);
  std::vector<Sample> samples((size_t)n);
  for (size_t i = 0; i < keys.size(); ++i)
    if (i < (size_t)n_common) {
      for (Sample& s : samples) s.push_back(keys[i]);
    } else {
      const int absent = (int)rnd((uint32_t)n);
      for (int s = 0; s < n; ++s)
        if (s != absent && rnd(2)) samples[(size_t)s].push_back(keys[i]);
    }
  for (Sample& s : samples) order(s, chrom_order);
  return samples;
}

static void check_ok(const char* name, const std::vector<Sample>& samples, long long want_common) {
  std::map<Key, int> seen;
  for (const Sample& s : samples)
    for (const Key& k : s) ++seen[k];
  const Result r = run(samples);
  CHECK(r.refusal.kind == 0, "%s: refused, kind %d sample %d site %lld", name, r.refusal.kind, r.refusal.sample, r.refusal.site);
  long long common = 0;
  for (const auto& kv : seen) common += kv.second == (int)samples.size();
  CHECK(r.n_common == common, "%s: n_common %lld, expected %lld", name, r.n_common, common);
  CHECK(want_common < 0 || common == want_common, "%s: the case has %lld common keys, not %lld", name, common, want_common);
  size_t i = 0;
  for (const Sample& s : samples) {
    long long kept = 0;
    for (const Key& k : s) {
      const uint8_t want = seen[k] == (int)samples.size() ? 1 : 0;
      CHECK(r.keep[i] == want, "%s: keep[%zu] = %d, expected %d", name, i, r.keep[i], want);
      kept += r.keep[i++];
    }
    CHECK(kept == common, "%s: a sample keeps %lld of %lld", name, kept, common);
  }
}

static void check_refused(const char* name, const std::vector<Sample>& samples, int kind, int sample, long long site) {
  const Result r = run(samples);
  CHECK(r.n_common == -1 && r.refusal.kind == kind + 1 && r.refusal.sample == sample && r.refusal.site == site,
        "%s: n_common %lld, kind %d sample %d site %lld; expected kind %d sample %d site %lld", name, r.n_common,
        r.refusal.kind, r.refusal.sample, r.refusal.site, kind + 1, sample, site);
  CHECK(!abn::common_refusal_text(r.refusal).empty(), "%s: no text", name);
}

int main() {
  const std::vector<int32_t> plain = {1, 10, 2}, organelles = {2, 1, 257, 256, 0, 255};
  int cases = 0;
  for (int n : {1, 2, 3, 5})
    for (int n_common : {0, 1, 63, 64, 65, 255, 256, 257, 1025})
      for (int n_extra : {0, 9, 200}) {
        char name[64];
        std::snprintf(name, sizeof name, "n %d common %d extra %d", n, n_common, n_extra);
        check_ok(name, make(n, n_common, n_extra, (n + n_common) % 2 ? plain : organelles), n_common);
        ++cases;
      }
  auto key = [](uint32_t i, int32_t c) { return Key{c, 10 + i, 11 + i, i % 3}; };
  Sample big;
  for (uint32_t i = 0; i < 3000; ++i) big.push_back(key(i, 1));
  check_ok("one empty sample", {Sample{}}, 0);
  check_ok("empty samples only", {Sample{}, Sample{}, Sample{}}, 0);
  check_ok("an empty sample among others", {Sample(big.begin(), big.begin() + 10), Sample{}, big}, 0);
  check_ok("1 and 3000, common", {Sample{big[1234]}, big}, 1);
  check_ok("3000 and 1, common", {big, Sample{big[2999]}}, 1);
  check_ok("1 and 3000, not common", {Sample{Key{1, 5, 5, 0}}, big}, 0);
  check_ok("a chromosome missing from one", {Sample{key(0, 1), key(1, 1), key(0, 2)}, Sample{key(0, 1), key(1, 1)}}, 2);
  check_ok("only end / strand differ", {Sample{Key{1, 5, 6, 0}, Key{1, 5, 6, 2}, Key{1, 5, 7, 0}}, Sample{Key{1, 5, 6, 1}, Key{1, 5, 7, 0}}}, 1);
  check_ok("the highest keys", {Sample{Key{257, 0xffffffffu, 0xffffffffu, 2}}, Sample{Key{257, 0xfffffffeu, 0xffffffffu, 2}, Key{257, 0xffffffffu, 0xffffffffu, 2}}}, 1);
  cases += 9;

  const Sample a = {key(0, 1), key(1, 1), key(2, 1), key(0, 10), key(1, 10), key(0, 2), key(1, 2)};
  Sample split = a;
  std::swap(split[2], split[3]);  // 1 1 10 1 10 2 2
  check_refused("split run", {a, split}, abn::kCommonSplitRun, 1, 3);
  Sample tail = a;
  tail.push_back(key(9, 1));
  check_refused("split run at the last site", {tail, a}, abn::kCommonSplitRun, 0, 7);
  Sample desc = a;
  std::swap(desc[0], desc[1]);
  check_refused("descending at site 1", {a, a, desc}, abn::kCommonNotAscending, 2, 1);
  Sample dup = a;
  dup.push_back(a.back());
  check_refused("duplicate at the last site", {dup}, abn::kCommonNotAscending, 0, 7);
  const Sample swapped = {key(0, 2), key(1, 2), key(0, 1), key(1, 1), key(2, 1), key(0, 10), key(1, 10), key(5, 10)};
  check_refused("the runs in another order", {a, swapped}, abn::kCommonNotCoordered, 1, 0);
  check_refused("a chromosome outside 0..257", {Sample{key(0, 1), key(0, 258)}}, abn::kCommonBadKey, 0, 1);
  check_refused("a strand above 2", {Sample{Key{1, 1, 1, 3}}}, abn::kCommonBadKey, 0, 0);
  cases += 7;
  if (failures) {
    std::printf("%d failures\n", failures);
    return 1;
  }
  std::printf("sanitized common sites ok: %d cases\n", cases);
  return 0;
}
