// Stand-alone driver for the pedigree build from resident sites (alphabeta_rs_amd/csrc/abn_codes.hpp), built by
// tests/test_codes_cpu.py with AddressSanitizer + UndefinedBehaviorSanitizer and run directly.  Seeded samples of 0, 1, 15,
// 16, 17, 255, 256 and 257 sites — no deferred line, inserted lines at the edges of chunks, adjacent ones, every site
// inserted, NaN posteriors on inserted lines, -0.0 levels — through codes_build_serial at chunk lengths 1, 2, 3, 64 and
// whole-file, rows of the sample's own stride and of a longer sample's, every chunk's arrays and every output in a heap
// block of exactly its length (a read or write past either end is a report), against a merge by line number, a
// field-by-field pack and a plain `if counted` fold written out here.  No device.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "../../alphabeta_rs_amd/csrc/abn_codes.hpp"

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

enum Kind { Record, Accepted, Rejected, Nothing };
struct Line {
  Kind kind;
  uint32_t status;
  double pm, ml;
};
struct ChunkData {
  std::unique_ptr<uint32_t[]> line, meta;
  std::unique_ptr<double[]> pm, ml;
};

int main() {
  const double filter = 0.99;
  static const long long kSites[8] = {0, 1, 15, 16, 17, 255, 256, 257};
  size_t sites = 0, inserted = 0, nan_posteriors = 0, neg_zero = 0, padded = 0, adjacent = 0;
  for (int it = 0; it < 96; ++it) {
    const int pattern = it % 6;
    const long long n_sites = kSites[(it / 6) % 8];
    // line 0 is the header; the sites are the first n_sites of a shuffle of the other lines
    const long long n_lines = 1 + n_sites + rnd((uint32_t)(n_sites / 4 + 3));
    std::vector<Line> file((size_t)n_lines);
    for (auto& l : file) l = Line{rnd(3) ? Nothing : Rejected, rnd(3), rnd(5) < 2 ? filter : rnd(1000) / 1000.0, rnd(1000) / 1000.0};
    std::vector<long long> order;
    for (long long i = 1; i < n_lines; ++i) order.push_back(i);
    for (size_t i = order.size(); i > 1; --i) std::swap(order[i - 1], order[rnd((uint32_t)i)]);
    for (long long k = 0; k < n_sites; ++k) file[(size_t)order[(size_t)k]].kind = Record;
    for (long long i = 1; i < n_lines; ++i) {
      Line& l = file[(size_t)i];
      if (l.kind != Record) continue;
      if (pattern == 1 && (i % 64 == 0 || i % 64 == 63 || i % 3 == 0)) l.kind = Accepted;
      if (pattern == 2 && rnd(12) == 0) {
        l.kind = Accepted;
        if (i + 1 < n_lines && file[(size_t)i + 1].kind == Record) file[(size_t)i + 1].kind = Accepted;
      }
      if (pattern == 3) l.kind = Accepted;
      if (pattern == 4 && rnd(3) == 0) l.kind = Accepted;
      if (pattern == 5 || rnd(4) == 0) l.ml = -0.0;
    }
    for (auto& l : file)
      if (l.kind == Accepted && rnd(3) == 0) l.pm = std::nan("");
    file[0].kind = Nothing;
    // the model: the merge by line number, the field of every site, the fold
    std::vector<uint8_t> want_field;
    std::vector<double> want_level;
    double want_sum = 0.0;
    long long want_kept = 0, prev_inserted = -2;
    std::vector<long long> iline;
    std::vector<uint8_t> istatus;
    std::vector<double> ipm, iml;
    for (long long i = 0; i < n_lines; ++i) {
      const Line& l = file[(size_t)i];
      if (l.kind != Record && l.kind != Accepted) continue;
      want_field.push_back(l.pm < filter ? 3 : (uint8_t)l.status);
      want_level.push_back(l.ml);
      if (l.pm >= filter) {
        want_sum += l.ml;
        ++want_kept;
      }
      nan_posteriors += l.pm != l.pm;
      neg_zero += std::signbit(l.ml) ? 1 : 0;
      if (l.kind == Accepted) {
        iline.push_back(i), istatus.push_back((uint8_t)l.status), ipm.push_back(l.pm), iml.push_back(l.ml);
        adjacent += prev_inserted + 1 == i;
        prev_inserted = i;
      }
    }
    sites += want_field.size();
    inserted += iline.size();
    const long long own = std::max<long long>((n_sites + 255) / 256 * 64, 64);
    for (long long stride : {own, own + 64}) {
      for (long long chunk_lines : {1LL, 2LL, 3LL, 64LL, n_lines}) {
        std::vector<ChunkData> data;
        std::vector<abn::MergeChunk> chunks;
        long long before = 0;
        for (long long line0 = 0; line0 < n_lines; line0 += chunk_lines) {
          const long long lines = std::min(chunk_lines, n_lines - line0);
          std::vector<uint32_t> line, meta;
          std::vector<double> pm, ml;
          for (long long i = line0; i < line0 + lines; ++i) {
            const Line& l = file[(size_t)i];
            if (l.kind != Record) continue;
            line.push_back((uint32_t)(i - line0));
            meta.push_back(5u | 2u << 16 | l.status << 20 | 1u << 24);
            pm.push_back(l.pm), ml.push_back(l.ml);
          }
          data.push_back(ChunkData{exact(line), exact(meta), exact(pm), exact(ml)});
          const ChunkData& d = data.back();
          chunks.push_back(abn::MergeChunk{d.line.get(), d.meta.get(), nullptr, nullptr, d.pm.get(), d.ml.get(),
                                           (long long)line.size(), line0, lines, before});
          before += (long long)line.size();
        }
        const auto xchunks = exact(chunks);
        const auto xline = exact(iline);
        std::unique_ptr<int32_t[]> pick(new int32_t[iline.size()]);
        if (!abn::merge_pick_chunks(xchunks.get(), (int)chunks.size(), xline.get(), (long long)iline.size(), pick.get())) {
          std::printf("iteration %d: a line in no chunk\n", it);
          return 1;
        }
        const auto xstatus = exact(istatus);
        const auto xpm = exact(ipm), xml = exact(iml);
        const abn::MergeInserted ins{xline.get(), pick.get(), nullptr, nullptr, nullptr, nullptr, xstatus.get(), xpm.get(),
                                     xml.get(), (long long)iline.size()};
        const size_t T = want_field.size();
        std::unique_ptr<uint8_t[]> code(new uint8_t[T]), row(new uint8_t[(size_t)stride]);
        std::unique_ptr<double[]> level(new double[T]);
        std::memset(row.get(), 0x5a, (size_t)stride);
        double sum = -1.0;
        long long kept = -1;
        abn::codes_build_serial(xchunks.get(), (int)chunks.size(), ins, filter, abn::CodesOut{code.get(), level.get()},
                                row.get(), stride, &sum, &kept);
        bool ok = kept == want_kept && (std::memcmp(&sum, &want_sum, 8) == 0 || (sum != sum && want_sum != want_sum));
        for (long long k = 0; k < 4 * stride && ok; ++k) {  // every field of the row, the padding's included
          const unsigned got = (row[(size_t)((k >> 4) * 4 + (k & 3))] >> (2 * ((k >> 2) & 3))) & 3u;
          ok = got == (k < (long long)T ? want_field[(size_t)k] : 3u);
        }
        for (size_t k = 0; k < T && ok; ++k) ok = std::memcmp(&level[k], &want_level[k], 8) == 0;
        if (!ok) {
          std::printf("iteration %d, %lld sites, chunks of %lld lines, stride %lld: the row, the levels or the fold differ\n",
                      it, n_sites, chunk_lines, stride);
          return 1;
        }
      }
      padded += (size_t)(4 * stride) > want_field.size();
    }
  }
  if (!sites || !inserted || !nan_posteriors || !neg_zero || !padded || !adjacent) {
    std::printf("the cases miss a pattern: %zu %zu %zu %zu %zu %zu\n", sites, inserted, nan_posteriors, neg_zero, padded,
                adjacent);
    return 1;
  }
  std::printf("sanitized codes build ok: %zu sites, %zu inserted, %zu NaN posteriors, %zu levels of -0.0\n", sites, inserted,
              nan_posteriors, neg_zero);
  return 0;
}
