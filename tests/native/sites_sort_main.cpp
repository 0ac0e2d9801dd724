// The sort of a resident methylome by genomic position (alphabeta_rs_amd/csrc/abn_sites_sort.hpp) in its serial forms,
// built plain and with -fsanitize=address,undefined by tests/test_sites_sort_cpu.py: every array a heap block of exactly
// its length.  The walk of the passes as the kernels make them — tile histograms, row scans, ranks from per-wavefront
// counts — against the stable comparison sort, with and without the pass skip; the flatten against a merge by line and
// the gather against the permutation, record for record.
#include <cstdio>
#include <cstring>
#include <memory>
#include <random>
#include <vector>

#include "../../alphabeta_rs_amd/csrc/abn_sites_sort.hpp"

using namespace abn;

namespace {

int fail(const char* what, long long a, long long b, long long c) {
  std::printf("FAILED: %s (%lld, %lld, %lld)\n", what, a, b, c);
  return 1;
}

struct Keys {  // four arrays of exactly n entries
  std::unique_ptr<int32_t[]> chromosome;
  std::unique_ptr<uint32_t[]> start, end;
  std::unique_ptr<uint8_t[]> strand;
  long long n;
  explicit Keys(long long count) : n(count) {
    const size_t k = (size_t)count;
    chromosome.reset(new int32_t[k]), start.reset(new uint32_t[k]), end.reset(new uint32_t[k]), strand.reset(new uint8_t[k]);
  }
};

// kind 0: three values per field; 1: the full ranges; 2: all equal; 3: ascending; 4: descending; 5: a methylome's shape
// (chromosomes 1..5, short sites) sorted by (chromosome, strand, start)
Keys make_keys(long long n, int kind, std::mt19937_64& rng) {
  Keys k(n);
  for (long long i = 0; i < n; ++i) {
    const size_t j = (size_t)i;
    switch (kind) {
      case 0:
        k.chromosome[j] = (int32_t)(rng() % 3), k.start[j] = (uint32_t)(rng() % 3), k.end[j] = (uint32_t)(rng() % 3);
        k.strand[j] = (uint8_t)(rng() % 3);
        break;
      case 1:
        k.chromosome[j] = (int32_t)(rng() % 258), k.start[j] = (uint32_t)rng(), k.end[j] = (uint32_t)rng();
        k.strand[j] = (uint8_t)(rng() % 3);
        break;
      case 2: k.chromosome[j] = 7, k.start[j] = 1000u, k.end[j] = 1001u, k.strand[j] = 1; break;
      case 3:
      case 4: {
        const long long v = kind == 3 ? i : n - 1 - i;
        k.chromosome[j] = (int32_t)(v / 1000), k.start[j] = (uint32_t)(v % 1000) * 3u, k.end[j] = k.start[j] + 1u;
        k.strand[j] = 0;
        break;
      }
      default: {
        const long long per = n / 5 + 1, within = i % per, half = per / 2 + 1;
        k.chromosome[j] = (int32_t)(1 + i / per), k.strand[j] = (uint8_t)(within / half);
        k.start[j] = (uint32_t)(within % half) * 2u + k.strand[j], k.end[j] = k.start[j] + 1u;
      }
    }
  }
  return k;
}

int run_keys(long long n, int kind, std::mt19937_64& rng, long long* placed) {
  const Keys k = make_keys(n, kind, rng);
  const size_t N = (size_t)n;
  std::unique_ptr<SortPair[]> ref(new SortPair[N]), a(new SortPair[N]), b(new SortPair[N]);
  const SortCheck check = sort_check_serial(n, k.chromosome.get(), k.start.get(), k.end.get(), k.strand.get(), ref.get());
  if (check.bad) return fail("a valid key counted as bad", n, kind, check.bad);
  long long descents = 0, equal = 0;
  for (long long i = 1; i < n; ++i) {
    const int c = sort_key_compare(ref[(size_t)i].w, ref[(size_t)i - 1].w);
    descents += c < 0, equal += c == 0;
  }
  if (descents != check.descents || equal != check.equal) return fail("the check's counts", n, kind, descents);
  if ((kind == 2 || kind == 3) && check.descents != 0) return fail("a descent in an ordered input", n, kind, check.descents);
  for (int skip = 0; skip < 2; ++skip) {
    std::memcpy(a.get(), ref.get(), sizeof(SortPair) * N);
    int passes = 0;
    const SortPair* got = sort_walk_serial(a.get(), b.get(), n, check, skip != 0, &passes);
    if (skip && passes != sort_passes_needed(check)) return fail("sort_passes_needed", n, kind, passes);
    if (!skip && passes != (check.descents ? kSortPasses : 0)) return fail("every pass of an unsorted input", n, kind, passes);
    std::unique_ptr<SortPair[]> want(new SortPair[N]);
    std::memcpy(want.get(), ref.get(), sizeof(SortPair) * N);
    sort_pairs_serial(want.get(), n);
    for (long long i = 0; i < n; ++i)
      if (got[i].index != want[(size_t)i].index || std::memcmp(got[i].w, want[(size_t)i].w, 12))
        return fail("the walk is not the stable sort", n, kind * 10 + skip, i);
    *placed += n;
  }
  return 0;
}

// chunks of chunk_n records with inserted records between them -> flatten, sort, gather, against the merge by line
int run_handle(const std::vector<long long>& chunk_n, long long n_ins_per_chunk, std::mt19937_64& rng, long long* placed) {
  const int n_chunks = (int)chunk_n.size();
  struct Block {
    std::unique_ptr<uint32_t[]> line, meta, start, end;
    std::unique_ptr<double[]> pm, ml;
  };
  std::vector<Block> src((size_t)n_chunks);
  std::vector<MergeChunk> chunks((size_t)n_chunks);
  std::vector<long long> iline;
  std::vector<int32_t> ichunk, ichrom;
  std::vector<uint32_t> istart, iend;
  std::vector<uint8_t> istrand, istatus, ictx;
  std::vector<double> ipm, iml;
  struct Rec {
    long long line;
    uint32_t meta, start, end;
    double pm, ml;
  };
  std::vector<Rec> all;  // in file order
  long long line0 = 0, before = 0;
  for (int c = 0; c < n_chunks; ++c) {
    const long long n = chunk_n[(size_t)c], n_lines = 2 * n + n_ins_per_chunk + 1;
    const size_t k = (size_t)n;
    Block& b = src[(size_t)c];
    b.line.reset(new uint32_t[k]), b.meta.reset(new uint32_t[k]), b.start.reset(new uint32_t[k]), b.end.reset(new uint32_t[k]);
    b.pm.reset(new double[k]), b.ml.reset(new double[k]);
    for (long long i = 0; i < n; ++i) {
      b.line[(size_t)i] = (uint32_t)(2 * i + 1);
      b.meta[(size_t)i] = (uint32_t)(rng() % 6) | (uint32_t)(rng() % 3) << 16 | (uint32_t)(rng() % 3) << 20 |
                          (uint32_t)(rng() % 16 == 0) << 24 | (uint32_t)(rng() % 4) << kMetaContextShift;
      b.start[(size_t)i] = (uint32_t)(rng() % 50), b.end[(size_t)i] = b.start[(size_t)i] + (uint32_t)(rng() % 3);
      b.pm[(size_t)i] = (double)(rng() % 10000) / 1e4, b.ml[(size_t)i] = (double)(rng() % 10000) / 1e4;
    }
    chunks[(size_t)c] = MergeChunk{b.line.get(), b.meta.get(), b.start.get(), b.end.get(), b.pm.get(), b.ml.get(), n, line0, n_lines, before};
    // the inserted lines of this slab: even slab lines (the records hold the odd ones), and the lines behind the records
    long long i = 0;
    for (long long j = 0; j < n_ins_per_chunk; ++j) {
      const long long rel = j < n ? 2 * j : 2 * n + 1 + (j - n);
      for (; i < n && b.line[(size_t)i] < rel; ++i)
        all.push_back(Rec{line0 + b.line[(size_t)i], b.meta[(size_t)i], b.start[(size_t)i], b.end[(size_t)i], b.pm[(size_t)i], b.ml[(size_t)i]});
      iline.push_back(line0 + rel), ichunk.push_back(c), ichrom.push_back((int32_t)(rng() % 6));
      istart.push_back((uint32_t)(rng() % 50)), iend.push_back(istart.back() + 1u), istrand.push_back((uint8_t)(rng() % 3));
      istatus.push_back((uint8_t)(rng() % 3)), ictx.push_back((uint8_t)(rng() % 4));
      ipm.push_back((double)(rng() % 10000) / 1e4), iml.push_back((double)(rng() % 10000) / 1e4);
      all.push_back(Rec{iline.back(), sort_inserted_meta(ichrom.back(), istrand.back(), istatus.back(), ictx.back()),
                        istart.back(), iend.back(), ipm.back(), iml.back()});
    }
    for (; i < n; ++i)
      all.push_back(Rec{line0 + b.line[(size_t)i], b.meta[(size_t)i], b.start[(size_t)i], b.end[(size_t)i], b.pm[(size_t)i], b.ml[(size_t)i]});
    line0 += n_lines, before += n;
  }
  const long long n = (long long)all.size();
  const size_t N = (size_t)n;
  for (size_t i = 1; i < N; ++i)
    if (all[i].line <= all[i - 1].line) return fail("the test's own file order", n, (long long)i, 0);
  const MergeInserted ins{iline.data(), ichunk.data(), ichrom.data(), istart.data(), iend.data(), istrand.data(),
                          istatus.data(), ipm.data(), iml.data(), (long long)iline.size()};
  std::unique_ptr<uint32_t[]> fmeta(new uint32_t[N]), fstart(new uint32_t[N]), fend(new uint32_t[N]);
  std::unique_ptr<double[]> fpm(new double[N]), fml(new double[N]);
  const SortFlat flat{fmeta.get(), fstart.get(), fend.get(), fpm.get(), fml.get()};
  std::memset(fmeta.get(), 0xff, 4 * N);
  sort_flatten_serial(chunks.data(), n_chunks, ins, ictx.data(), flat);
  for (size_t i = 0; i < N; ++i)
    if (fmeta[i] != all[i].meta || fstart[i] != all[i].start || fend[i] != all[i].end || std::memcmp(&fpm[i], &all[i].pm, 8) ||
        std::memcmp(&fml[i], &all[i].ml, 8))
      return fail("the flatten is not the merge by line", n, (long long)i, 0);
  std::unique_ptr<SortPair[]> a(new SortPair[N]), b(new SortPair[N]);
  SortCheck check;
  for (long long i = 0; i < n; ++i) {  // the check over the flattened records, as SortKeysMeta reads them
    const SortKey k = sort_key_of_meta(fmeta[(size_t)i], fstart[(size_t)i], fend[(size_t)i]);
    a[(size_t)i] = SortPair{{k.w[0], k.w[1], k.w[2]}, (uint32_t)i};
    for (int j = 0; j < 3; ++j) check.key_or[j] |= k.w[j], check.key_and[j] &= k.w[j];
    if (i > 0) check.descents += sort_key_compare(a[(size_t)i].w, a[(size_t)i - 1].w) < 0;
  }
  int passes = 0;
  const SortPair* got = sort_walk_serial(a.get(), b.get(), n, check, true, &passes);
  std::unique_ptr<uint32_t[]> order(new uint32_t[N]), oline(new uint32_t[N]), ometa(new uint32_t[N]), ostart(new uint32_t[N]),
      oend(new uint32_t[N]);
  std::unique_ptr<double[]> opm(new double[N]), oml(new double[N]);
  for (size_t i = 0; i < N; ++i) order[i] = got[i].index;
  const ParseRecords out{oline.get(), ometa.get(), ostart.get(), oend.get(), opm.get(), oml.get()};
  for (long long k = 0; k < n; ++k) sort_gather_record(flat, order.get(), k, n, out);
  for (size_t k = 0; k < N; ++k) {
    const Rec& r = all[order[k]];
    if (oline[k] != (uint32_t)k || ometa[k] != r.meta || ostart[k] != r.start || oend[k] != r.end || std::memcmp(&opm[k], &r.pm, 8) ||
        std::memcmp(&oml[k], &r.ml, 8))
      return fail("a gathered record", n, (long long)k, 0);
    if (k > 0) {
      const SortKey p = sort_key_of_meta(ometa[k - 1], ostart[k - 1], oend[k - 1]), q = sort_key_of_meta(ometa[k], ostart[k], oend[k]);
      const int c = sort_key_compare(q.w, p.w);
      if (c < 0 || (c == 0 && order[k] < order[k - 1])) return fail("the gathered records are not in canonical order", n, (long long)k, c);
    }
  }
  *placed += n;
  return 0;
}

}  // namespace

int main() {
  std::mt19937_64 rng(20240611);
  long long placed = 0, cases = 0;
  // every one of the 75 key bits is read by exactly one pass, least significant first over (strand, end, start, chromosome)
  for (int bit = 0; bit < kSortKeyBits; ++bit) {
    uint32_t chrom = 0, start = 0, end = 0, strand = 0;
    if (bit < 2) strand = 1u << bit;
    else if (bit < 34) end = 1u << (bit - 2);
    else if (bit < 66) start = 1u << (bit - 34);
    else chrom = 1u << (bit - 66);
    const SortKey k = sort_key(chrom, start, end, strand);
    for (int p = 0; p < kSortPasses; ++p) {
      const uint32_t want = p == bit / kSortDigitBits ? 1u << (bit % kSortDigitBits) : 0u;
      if (sort_digit(k.w, p) != want) return fail("sort_digit", bit, p, sort_digit(k.w, p));
    }
  }
  const long long sizes[] = {0, 1, 2, 63, 64, 65, kSortTile - 1, kSortTile, kSortTile + 1, 3 * kSortTile + 17};
  for (long long n : sizes)
    for (int kind = 0; kind < 6; ++kind) {
      if (run_keys(n, kind, rng, &placed)) return 1;
      ++cases;
    }
  const long long counts[] = {0, 1, 255, 257, 1025};
  for (long long a : counts)
    for (long long b : counts)
      for (long long n_ins : {0ll, 1ll, 7ll}) {
        if (run_handle({a, b}, n_ins, rng, &placed) || run_handle({0, a, 0, b, 300}, n_ins, rng, &placed)) return 1;
        cases += 2;
      }
  if (run_handle({}, 0, rng, &placed)) return 1;
  std::printf("sites sort ok: %lld cases, %lld records placed\n", cases + 1, placed);
  return 0;
}
