// The collapse of a resident methylome's repeated sites (alphabeta_rs_amd/csrc/abn_sites_dedup.hpp) in its serial forms,
// built plain and with -fsanitize=address,undefined by tests/test_sites_dedup_cpu.py: every array a heap block of exactly
// its length.  The walk of the kernels' structure — the flags lane by lane with the workgroups' striding, BEST's walk from
// the lane of the run's head, the tile counts, their scan and the scatter's ranks from the groups' counts — against the
// serial form run after run, under all four policies, through both record layouts (the primitive's arrays and a flattened
// sample's meta words); and the gather against the kept indices, record for record.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <memory>
#include <random>
#include <vector>

#include "../../alphabeta_rs_amd/csrc/abn_sites_dedup.hpp"

using namespace abn;

namespace {

int fail(const char* what, long long a, long long b, long long c) {
  std::printf("FAILED: %s (%lld, %lld, %lld)\n", what, a, b, c);
  return 1;
}

struct Records {  // arrays of exactly n entries
  std::unique_ptr<int32_t[]> chromosome;
  std::unique_ptr<uint32_t[]> start, end, meta;
  std::unique_ptr<uint8_t[]> strand, status;
  std::unique_ptr<double[]> pm, ml;
  long long n;
  explicit Records(long long count) : n(count) {
    const size_t k = (size_t)count;
    chromosome.reset(new int32_t[k]), start.reset(new uint32_t[k]), end.reset(new uint32_t[k]), meta.reset(new uint32_t[k]);
    strand.reset(new uint8_t[k]), status.reset(new uint8_t[k]), pm.reset(new double[k]), ml.reset(new double[k]);
  }
  DedupArrays arrays() const {
    return DedupArrays{chromosome.get(), start.get(), end.get(), strand.get(), pm.get(), status.get()};
  }
  DedupMeta by_meta() const { return DedupMeta{meta.get(), start.get(), end.get(), pm.get()}; }
};

// the length of the next run.  kind 0: no repeats; 1: all equal; 2: pairs; 3: random 1..5; 4: a run of two begins at
// records 63, 127, ..; 5: one run of 2 * kSortTile + 5 in the middle; 6: a run of three at the start and at the end
long long run_length(long long n, int kind, long long at, std::mt19937_64& rng) {
  switch (kind) {
    case 0: return 1;
    case 1: return n;
    case 2: return 2;
    case 3: return 1 + (long long)(rng() % 5);
    case 4: return at % 64 == 63 ? 2 : 1;
    case 5: return at == (n - (2 * kSortTile + 5)) / 2 && n > 2 * kSortTile + 5 ? 2 * kSortTile + 5 : 1;
    default: return at == 0 || at == n - 3 ? 3 : 1;
  }
}

Records make_records(long long n, int kind, std::mt19937_64& rng) {
  const double values[] = {std::numeric_limits<double>::quiet_NaN(), -0.0, 0.0, 0.5, 0.5, 0.75, 0.99, 0.99, 1.0};
  Records r(n);
  long long key = 0;
  for (long long at = 0; at < n; ++key) {
    long long len = run_length(n, kind, at, rng);
    if (len > n - at) len = n - at;
    const bool all_nan = kind == 3 && key % 3 == 0;
    for (long long i = at; i < at + len; ++i) {
      const size_t j = (size_t)i;
      r.chromosome[j] = key * 3 / (n + 1) == 0 ? 0 : (key * 3 / (n + 1) == 1 ? 256 : 257);
      r.start[j] = 100u + 3u * (uint32_t)(key / 2), r.end[j] = r.start[j] + 1u;
      r.strand[j] = (uint8_t)((key % 2) * 2);
      r.status[j] = (uint8_t)(rng() % 3);
      r.pm[j] = all_nan ? values[0] : values[rng() % 9];
      r.ml[j] = (double)i;
      r.meta[j] = (uint32_t)r.chromosome[j] | (uint32_t)r.strand[j] << 16 | (uint32_t)r.status[j] << 20 | (uint32_t)(rng() % 3) << kMetaContextShift;
    }
    at += len;
  }
  return r;
}

template <class Keys>
int run_policy(const Keys& keys, const Records& r, int kind, int policy, long long* kept_all) {
  const long long n = r.n;
  const size_t N = (size_t)n;
  std::unique_ptr<long long[]> want(new long long[N]), got(new long long[N]);
  long long info[4] = {-1, -1, -1, -1}, descent = 0;
  if (dedup_serial(keys, n, policy, want.get(), info, &descent) != 0 || descent != -1) return fail("a refusal of a valid input", n, kind, policy);
  if (info[0] != n || info[1] < 0 || info[1] > n) return fail("the serial form's counts", n, kind, info[1]);
  // the serial form against the definition: strictly ascending, one record per run (none of a repeated key under DROP),
  // and under BEST no record of the run is better than the kept one, no earlier one as good
  for (long long k = 0; k < info[1]; ++k) {
    if (want[(size_t)k] < 0 || want[(size_t)k] >= n || (k > 0 && want[(size_t)k] <= want[(size_t)k - 1])) return fail("the kept indices ascend", n, kind, k);
    if (k > 0) {
      const SortKey a = keys.key(want[(size_t)k]), b = keys.key(want[(size_t)k - 1]);
      if (sort_key_compare(a.w, b.w) <= 0) return fail("a key kept twice", n, kind, k);
    }
    if (policy == kDedupBest) {
      const long long at = want[(size_t)k];
      const SortKey a = keys.key(at);
      for (long long j = at - 1; j >= 0; --j) {
        const SortKey b = keys.key(j);
        if (sort_key_compare(a.w, b.w) != 0) break;
        const double x = keys.posterior(j), y = keys.posterior(at);
        if (!(y > x || (std::isnan(x) && !std::isnan(y)))) return fail("an earlier record as good as the best", n, kind, at);
      }
      for (long long j = at + 1; j < n; ++j) {
        const SortKey b = keys.key(j);
        if (sort_key_compare(a.w, b.w) != 0) break;
        if (dedup_better(keys.posterior(j), keys.posterior(at))) return fail("a later record better than the best", n, kind, at);
      }
    }
  }
  for (long long blocks = 1; blocks <= 5; blocks += 2) {
    std::unique_ptr<uint8_t[]> keep(new uint8_t[N]);
    std::unique_ptr<uint32_t[]> count(new uint32_t[(size_t)sort_tiles(n) + 1]);
    std::memset(keep.get(), 0xee, N);  // a flag no lane wrote stays neither 0 nor 1
    const DedupCheck check = dedup_flags_walk(keys, n, policy, blocks, keep.get());
    for (size_t i = 0; i < N; ++i)
      if (keep[i] > 1) return fail("a keep flag without a writer", n, kind, (long long)i);
    if (check.descent != kDedupNoDescent || check.bad != 0) return fail("a descent or bad key in a valid input", n, kind, policy);
    if (check.repeated != info[2] || check.disagreeing != info[3]) return fail("the flags' counts", n, kind, policy);
    const long long kept = dedup_compact_walk(keep.get(), n, count.get(), got.get());
    if (kept != info[1]) return fail("the number kept", n, kind, kept);
    if (kept > 0 && std::memcmp(got.get(), want.get(), (size_t)kept * sizeof(long long)) != 0) return fail("the kept indices", n, kind, policy);
  }
  *kept_all += info[1];
  // the gather: the kept records, line = rank
  const size_t K = (size_t)info[1];
  std::unique_ptr<uint32_t[]> order(new uint32_t[K]), line(new uint32_t[K]), meta(new uint32_t[K]), start(new uint32_t[K]), end(new uint32_t[K]);
  std::unique_ptr<double[]> pm(new double[K]), ml(new double[K]);
  for (size_t k = 0; k < K; ++k) order[k] = (uint32_t)want[k];
  const SortFlat flat{r.meta.get(), r.start.get(), r.end.get(), r.pm.get(), r.ml.get()};
  const ParseRecords out{line.get(), meta.get(), start.get(), end.get(), pm.get(), ml.get()};
  for (long long k = 0; k < info[1]; ++k) dedup_gather_record(flat, order.get(), k, n, out);
  for (size_t k = 0; k < K; ++k) {
    const size_t i = (size_t)want[k];
    if (line[k] != k || meta[k] != r.meta[i] || start[k] != r.start[i] || end[k] != r.end[i] || ml[k] != r.ml[i] ||
        std::memcmp(&pm[k], &r.pm[i], sizeof(double)) != 0)
      return fail("the gathered record", n, kind, (long long)k);
  }
  return 0;
}

}  // namespace

int main() {
  std::mt19937_64 rng(20260101);
  const long long sizes[] = {0, 1, 2, 63, 64, 65, kSortTile - 1, kSortTile, kSortTile + 1, 3 * kSortTile + 17};
  long long cases = 0, kept = 0;
  for (long long n : sizes)
    for (int kind = 0; kind < 7; ++kind) {
      const Records r = make_records(n, kind, rng);
      for (int policy = kDedupFirst; policy <= kDedupDrop; ++policy) {
        if (run_policy(r.arrays(), r, kind, policy, &kept)) return 1;
        if (run_policy(r.by_meta(), r, kind, policy, &kept)) return 1;
        cases += 2;
      }
    }
  // refusals of the serial form: a descent is named, a bad key is not
  {
    Records r = make_records(100, 3, rng);
    std::unique_ptr<long long[]> order(new long long[100]);
    long long info[4], descent = 0;
    r.start[40] = 0u;
    if (dedup_serial(r.arrays(), r.n, kDedupBest, order.get(), info, &descent) != 1 || descent != 40) return fail("the descent", 100, descent, 0);
    const DedupCheck check = dedup_flags_walk(r.arrays(), r.n, kDedupBest, 2, std::unique_ptr<uint8_t[]>(new uint8_t[100]).get());
    if (check.descent != 40u) return fail("the flags' descent", 100, check.descent, 0);
    r.chromosome[3] = 258;
    if (dedup_serial(r.arrays(), r.n, kDedupFirst, order.get(), info, &descent) != 1 || descent != -1) return fail("the bad key", 100, descent, 0);
  }
  std::printf("sites dedup ok: %lld cases, %lld records kept\n", cases, kept);
  return 0;
}
