// Stand-alone driver for the union step (alphabeta_rs_amd/csrc/abn_sites_union.hpp), built by
// tests/test_sites_union_cpu.py with AddressSanitizer + UndefinedBehaviorSanitizer and run directly.  Seeded cases of 1 to 9
// samples — empty samples, a sample of one site beside one of 3000, chromosomes missing from a sample, the runs in the
// order 1, 10, 2 and 2, 1, 257, 256, 0, 255, identical and disjoint samples, union sizes on both sides of 64 and 256 —
// through sites_union_serial with its gather, every input and output array in a heap block of exactly its length (a read
// or write past either end is a report), against a union by sort and unique written out here; and samples with a split
// run, a descending neighbour, a key outside its range and the runs in another order, which must be refused at the
// expected site.  No device.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <memory>
#include <tuple>
#include <vector>

#include "../../alphabeta_rs_amd/csrc/abn_sites_union.hpp"

using Key = std::tuple<int32_t, uint32_t, uint32_t, uint32_t>;  // chromosome, start, end, strand
using Sample = std::vector<Key>;

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
  long long n_union = -1;
  abn::CommonRefusal refusal{0, -1, -1};
  std::vector<uint32_t> dest;
  std::vector<int32_t> chrom;  // the gathered rows, n x n_union
  std::vector<uint32_t> start, end;
  std::vector<uint8_t> strand, code;
  std::vector<double> level;
};

static uint8_t code_of(size_t i) { return (uint8_t)(i % 3 | 0x40); }
static double level_of(size_t i) { return (double)i + 0.25; }

static Result run(const std::vector<Sample>& samples) {
  const int n = (int)samples.size();
  std::vector<long long> off((size_t)n + 1, 0);
  std::vector<int32_t> chrom;
  std::vector<uint32_t> start, end;
  std::vector<uint8_t> strand, code;
  std::vector<double> level;
  for (int s = 0; s < n; ++s) {
    off[(size_t)s + 1] = off[(size_t)s] + (long long)samples[(size_t)s].size();
    for (const Key& k : samples[(size_t)s]) {
      code.push_back(code_of(chrom.size()));
      level.push_back(level_of(chrom.size()));
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
  const auto pcode = exact(code);
  const auto plevel = exact(level);
  std::unique_ptr<uint32_t[]> dest(new uint32_t[chrom.size()]);
  std::unique_ptr<int32_t[]> ochrom;
  std::unique_ptr<uint32_t[]> ostart, oend;
  std::unique_ptr<uint8_t[]> ostrand, ocode;
  std::unique_ptr<double[]> olevel;
  size_t A = 0;
  Result r;
  r.n_union = abn::sites_union_serial(
      abn::CommonSites{pchrom.get(), pstart.get(), pend.get(), pstrand.get()}, n, poff.get(), dest.get(), &r.refusal,
      [&](long long n_union) {
        A = (size_t)n * (size_t)n_union;
        ochrom.reset(new int32_t[A]), ostart.reset(new uint32_t[A]), oend.reset(new uint32_t[A]);
        ostrand.reset(new uint8_t[A]), ocode.reset(new uint8_t[A]), olevel.reset(new double[A]);
        return abn::CommonGather{pcode.get(), plevel.get(), ochrom.get(), ostart.get(), oend.get(), ostrand.get(),
                                 olevel.get(),  ocode.get(),  n_union};
      });
  if (r.n_union >= 0) {
    r.dest.assign(dest.get(), dest.get() + chrom.size());
    r.chrom.assign(ochrom.get(), ochrom.get() + A), r.start.assign(ostart.get(), ostart.get() + A);
    r.end.assign(oend.get(), oend.get() + A), r.strand.assign(ostrand.get(), ostrand.get() + A);
    r.code.assign(ocode.get(), ocode.get() + A), r.level.assign(olevel.get(), olevel.get() + A);
  }
  return r;
}

static bool before(const Key& a, const Key& b, const std::vector<int32_t>& chrom_order) {
  auto rank = [&](int32_t c) { return std::find(chrom_order.begin(), chrom_order.end(), c) - chrom_order.begin(); };
  if (std::get<0>(a) != std::get<0>(b)) return rank(std::get<0>(a)) < rank(std::get<0>(b));
  return std::tie(std::get<1>(a), std::get<2>(a), std::get<3>(a)) < std::tie(std::get<1>(b), std::get<2>(b), std::get<3>(b));
}

// the samples' keys ordered as the files are: the chromosomes in chrom_order, (start, end, strand) ascending inside
static void order(Sample& s, const std::vector<int32_t>& chrom_order) {
  std::sort(s.begin(), s.end(), [&](const Key& a, const Key& b) { return before(a, b, chrom_order); });
}

// n_all keys in every sample, n_extra keys in some and not in all (none for one sample), and a key per chromosome in the
// first sample alone
static std::vector<Sample> make(int n, int n_all, int n_extra, const std::vector<int32_t>& chrom_order) {
  Sample keys;
  const uint32_t span = (uint32_t)std::max(8, (n_all + n_extra) / 4);
  const size_t want = (size_t)n_all + (n > 1 ? (size_t)n_extra : 0);
  while (keys.size() < want) {
    const uint32_t s = 1 + rnd(span);
    const Key k{chrom_order[rnd((uint32_t)chrom_order.size())], s, s + rnd(3), rnd(3)};
    if (std::find(keys.begin(), keys.end(), k) == keys.end()) keys.push_back(k);
  }
  std::vector<Sample> samples((size_t)n);
  for (size_t i = 0; i < keys.size(); ++i)
    if (i < (size_t)n_all) {
      for (Sample& s : samples) s.push_back(keys[i]);
    } else {
      const int absent = (int)rnd((uint32_t)n), present = (absent + 1 + (int)rnd((uint32_t)n - 1)) % n;
      for (int s = 0; s < n; ++s)
        if (s == present || (s != absent && rnd(2))) samples[(size_t)s].push_back(keys[i]);
    }
  for (int32_t c : chrom_order) samples[0].push_back(Key{c, 0, 0, 0});  // sample 0 has every run: it is the reference
  for (Sample& s : samples) order(s, chrom_order);
  return samples;
}

// chrom_order: an order every sample's runs follow and whose first chromosomes are the reference sample's
static void check_ok(const char* name, const std::vector<Sample>& samples, const std::vector<int32_t>& chrom_order,
                     long long want_union) {
  Sample all;
  for (const Sample& s : samples) all.insert(all.end(), s.begin(), s.end());
  order(all, chrom_order);
  all.erase(std::unique(all.begin(), all.end()), all.end());
  const long long nu = (long long)all.size();
  const Result r = run(samples);
  CHECK(r.refusal.kind == 0, "%s: refused, kind %d sample %d site %lld", name, r.refusal.kind, r.refusal.sample, r.refusal.site);
  CHECK(r.n_union == nu, "%s: n_union %lld, expected %lld", name, r.n_union, nu);
  CHECK(want_union < 0 || nu == want_union, "%s: the case has %lld keys, not %lld", name, nu, want_union);
  if (r.n_union != nu) return;
  size_t i = 0;
  for (size_t s = 0; s < samples.size(); ++s) {
    std::vector<long long> mine((size_t)nu, -1);  // the sample's site at every rank
    for (const Key& k : samples[s]) {
      const long long u = std::lower_bound(all.begin(), all.end(), k, [&](const Key& a, const Key& b) { return before(a, b, chrom_order); }) - all.begin();
      CHECK(r.dest[i] == (uint32_t)u, "%s: dest[%zu] = %u, expected %lld", name, i, r.dest[i], u);
      mine[(size_t)u] = (long long)i++;
    }
    for (long long u = 0; u < nu; ++u) {
      const size_t d = s * (size_t)nu + (size_t)u;
      const Key got{r.chrom[d], r.start[d], r.end[d], r.strand[d]};
      CHECK(got == all[(size_t)u], "%s: sample %zu rank %lld: another key", name, s, u);
      const long long m = mine[(size_t)u];
      const uint8_t code = m < 0 ? (uint8_t)0x80 : code_of((size_t)m);
      const double level = m < 0 ? 0.0 : level_of((size_t)m);
      CHECK(r.code[d] == code, "%s: sample %zu rank %lld: code %d, expected %d", name, s, u, r.code[d], code);
      CHECK(std::memcmp(&r.level[d], &level, 8) == 0, "%s: sample %zu rank %lld: level %g, expected %g", name, s, u, r.level[d], level);
    }
  }
}

static void check_refused(const char* name, const std::vector<Sample>& samples, int kind, int sample, long long site) {
  const Result r = run(samples);
  CHECK(r.n_union == -1 && r.refusal.kind == kind && r.refusal.sample == sample && r.refusal.site == site,
        "%s: n_union %lld, kind %d sample %d site %lld; expected kind %d sample %d site %lld", name, r.n_union,
        r.refusal.kind, r.refusal.sample, r.refusal.site, kind, sample, site);
  CHECK(!abn::union_refusal_text(r.refusal).empty(), "%s: no text", name);
}

int main() {
  const std::vector<int32_t> plain = {1, 10, 2}, organelles = {2, 1, 257, 256, 0, 255};
  int cases = 0;
  for (int n : {1, 2, 3, 5, 6, 9})
    for (int n_all : {0, 1, 57, 64, 250, 1020})
      for (int n_extra : {0, 5, 6, 7, 200}) {
        char name[64];
        std::snprintf(name, sizeof name, "n %d all %d extra %d", n, n_all, n_extra);
        const std::vector<int32_t>& chroms = (n + n_all) % 2 ? plain : organelles;
        check_ok(name, make(n, n_all, n_extra, chroms), chroms, n_all + (n > 1 ? n_extra : 0) + (long long)chroms.size());
        ++cases;
      }
  auto key = [](uint32_t i, int32_t c) { return Key{c, 10 + i, 11 + i, i % 3}; };
  Sample big;
  for (uint32_t i = 0; i < 3000; ++i) big.push_back(key(i, 1));
  const Sample ten(big.begin(), big.begin() + 10), next(big.begin() + 5, big.begin() + 15);
  check_ok("one sample", {Sample(big.begin(), big.begin() + 300)}, plain, 300);
  check_ok("one empty sample", {Sample{}}, plain, 0);
  check_ok("empty samples only", {Sample{}, Sample{}, Sample{}}, plain, 0);
  check_ok("an empty sample among others", {ten, Sample{}, next}, plain, 15);
  check_ok("identical", {ten, ten, ten, ten, ten}, plain, 10);
  check_ok("disjoint", {Sample(big.begin(), big.begin() + 100), Sample(big.begin() + 100, big.begin() + 200)}, plain, 200);
  check_ok("1 and 3000", {Sample{big[1234]}, big}, plain, 3000);
  check_ok("3000 and 1 below all", {big, Sample{Key{1, 5, 5, 0}}}, plain, 3001);
  check_ok("a chromosome only the last has", {ten, ten, Sample{key(0, 1), key(1, 1), key(0, 2)}}, plain, 11);
  check_ok("only end / strand / chromosome differ",
           {Sample{Key{1, 5, 6, 0}, Key{1, 5, 6, 2}, Key{1, 5, 7, 0}}, Sample{Key{1, 5, 6, 1}, Key{1, 5, 7, 0}, Key{2, 5, 7, 0}}}, plain, 5);
  check_ok("the highest keys", {Sample{Key{257, 0xffffffffu, 0xffffffffu, 2}},
                                Sample{Key{257, 0xfffffffeu, 0xffffffffu, 2}, Key{257, 0xffffffffu, 0xffffffffu, 2}}}, organelles, 2);
  cases += 11;

  const Sample a = {key(0, 1), key(1, 1), key(2, 1), key(0, 10), key(1, 10), key(0, 2), key(1, 2)};
  Sample split = a;
  std::swap(split[2], split[3]);  // 1 1 10 1 10 2 2
  check_refused("split run", {a, split}, 1 + abn::kCommonSplitRun, 1, 3);
  Sample desc = a;
  std::swap(desc[0], desc[1]);
  check_refused("descending at site 1", {a, a, desc}, 1 + abn::kCommonNotAscending, 2, 1);
  Sample dup = a;
  dup.push_back(a.back());
  check_refused("duplicate at the last site", {dup}, 1 + abn::kCommonNotAscending, 0, 7);
  const Sample swapped = {key(0, 2), key(1, 2), key(0, 1), key(1, 1), key(2, 1), key(0, 10), key(1, 10), key(5, 10)};
  check_refused("the runs in another order", {a, swapped}, abn::kUnionRunOrder, 1, 2);
  check_refused("the runs in another order, the last run", {a, Sample{key(0, 1), key(0, 2), key(0, 10)}}, abn::kUnionRunOrder, 1, 2);
  check_refused("a chromosome outside 0..257", {a, Sample{key(0, 1), key(0, 258)}}, 1 + abn::kCommonBadKey, 1, 1);
  check_refused("a strand above 2", {Sample{Key{1, 1, 1, 3}}}, 1 + abn::kCommonBadKey, 0, 0);
  cases += 7;
  if (failures) {
    std::printf("%d failures\n", failures);
    return 1;
  }
  std::printf("sanitized union sites ok: %d cases\n", cases);
  return 0;
}
