// Stand-alone driver for the merge of the parser's records with the host-decided lines
// (alphabeta_rs_amd/csrc/abn_sites_merge.hpp), built by tests/test_sites_merge_cpu.py with AddressSanitizer +
// UndefinedBehaviorSanitizer and run directly.  Seeded files of up to 600 lines — no deferred line, every line deferred,
// the first and last line of a chunk, adjacent lines, a chunk without a record, deferred lines the host rejects, all of
// them rejected — through sites_merge_serial at chunk lengths 1, 2, 3, 64 and whole-file, every chunk's arrays and every
// output in a heap block of exactly its length (a read or write past either end is a report), against a merge by line
// number written out here.  No device.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "../../alphabeta_rs_amd/csrc/abn_sites_merge.hpp"

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
  int32_t chromosome;
  uint32_t start, end, strand, status, flag;
  double pm, ml;
};

struct ChunkData {
  std::unique_ptr<uint32_t[]> line, meta, start, end;
  std::unique_ptr<double[]> pm, ml;
};

int main() {
  const double filter = 0.99;
  size_t records = 0, inserted = 0, rejected = 0, empty_chunks = 0, nan_codes = 0;
  for (int it = 0; it < 300; ++it) {
    const int pattern = it % 8;
    const long long n_lines = 2 + rnd(600);  // line 0 is the header
    static const long long kOwn[4] = {1, 2, 3, 64};
    const long long own = kOwn[rnd(4)];
    std::vector<Line> file((size_t)n_lines);
    for (auto& l : file)
      l = Line{rnd(10) < 7 ? Record : Nothing, (int32_t)rnd(258), rnd(1u << 31) * 2u + rnd(2), rnd(1u << 31) * 2u + rnd(2),
               rnd(3), rnd(3), rnd(20) == 0 ? 1u : 0u, rnd(2) ? 0.99 : rnd(1000) / 1000.0, rnd(1000) / 1000.0};
    for (long long i = 0; i < n_lines; ++i) {
      Line& l = file[(size_t)i];
      if (pattern == 1) l.kind = Accepted;
      if (pattern == 2) l.kind = Rejected;
      if (pattern == 3 && (i % own == 0 || i % own == own - 1)) l.kind = rnd(3) ? Accepted : Rejected;
      if (pattern == 4 && rnd(40) == 0) {
        l.kind = Accepted;
        if (i + 1 < n_lines) file[(size_t)i + 1].kind = Accepted, ++i;
      }
      if (pattern == 5 && i / own == n_lines / own / 2) l.kind = rnd(2) ? Accepted : Nothing;
      if (pattern == 6) l.kind = (Kind)rnd(4);
      if (l.kind == Accepted && rnd(3) == 0) l.pm = std::nan("");
    }
    file[0].kind = Nothing;
    // the merge by line number
    std::vector<long long> place((size_t)n_lines, -1);
    long long total = 0;
    for (long long i = 0; i < n_lines; ++i)
      if (file[(size_t)i].kind == Record || file[(size_t)i].kind == Accepted) place[(size_t)i] = total++;
    std::vector<long long> iline;
    std::vector<int32_t> ichrom;
    std::vector<uint32_t> istart, iend;
    std::vector<uint8_t> istrand, istatus;
    std::vector<double> ipm, iml;
    for (long long i = 0; i < n_lines; ++i) {
      const Line& l = file[(size_t)i];
      rejected += l.kind == Rejected;
      if (l.kind != Accepted) continue;
      iline.push_back(i), ichrom.push_back(l.chromosome), istart.push_back(l.start), iend.push_back(l.end);
      istrand.push_back((uint8_t)l.strand), istatus.push_back((uint8_t)l.status), ipm.push_back(l.pm), iml.push_back(l.ml);
    }
    inserted += iline.size();
    for (long long chunk_lines : {1LL, 2LL, 3LL, 64LL, n_lines}) {
      std::vector<ChunkData> data;
      std::vector<abn::MergeChunk> chunks;
      long long before = 0;
      for (long long line0 = 0; line0 < n_lines; line0 += chunk_lines) {
        const long long lines = std::min(chunk_lines, n_lines - line0);
        std::vector<uint32_t> line, meta, start, end;
        std::vector<double> pm, ml;
        for (long long i = line0; i < line0 + lines; ++i) {
          const Line& l = file[(size_t)i];
          if (l.kind != Record) continue;
          line.push_back((uint32_t)(i - line0));
          meta.push_back((uint32_t)l.chromosome | l.strand << 16 | l.status << 20 | l.flag << 24);
          start.push_back(l.start), end.push_back(l.end), pm.push_back(l.pm), ml.push_back(l.ml);
        }
        empty_chunks += line.empty();
        data.push_back(ChunkData{exact(line), exact(meta), exact(start), exact(end), exact(pm), exact(ml)});
        const ChunkData& d = data.back();
        chunks.push_back(abn::MergeChunk{d.line.get(), d.meta.get(), d.start.get(), d.end.get(), d.pm.get(), d.ml.get(),
                                         (long long)line.size(), line0, lines, before});
        before += (long long)line.size();
      }
      if (chunk_lines == 1) records += (size_t)before;
      const auto xchunks = exact(chunks);
      const auto xline = exact(iline);
      std::unique_ptr<int32_t[]> pick(new int32_t[iline.size()]);
      if (!abn::merge_pick_chunks(xchunks.get(), (int)chunks.size(), xline.get(), (long long)iline.size(), pick.get())) {
        std::printf("iteration %d: a line in no chunk\n", it);
        return 1;
      }
      const auto xchrom = exact(ichrom);
      const auto xstart = exact(istart), xend = exact(iend);
      const auto xstrand = exact(istrand), xstatus = exact(istatus);
      const auto xpm = exact(ipm), xml = exact(iml);
      const abn::MergeInserted ins{xline.get(), pick.get(), xchrom.get(), xstart.get(), xend.get(), xstrand.get(),
                                   xstatus.get(), xpm.get(), xml.get(), (long long)iline.size()};
      const size_t T = (size_t)total;
      std::unique_ptr<int32_t[]> ochrom(new int32_t[T]);
      std::unique_ptr<uint32_t[]> ostart(new uint32_t[T]), oend(new uint32_t[T]);
      std::unique_ptr<uint8_t[]> ostrand(new uint8_t[T]), ocode(new uint8_t[T]);
      std::unique_ptr<double[]> olevel(new double[T]);
      std::unique_ptr<long long[]> dr(new long long[(size_t)before]), di(new long long[iline.size()]);
      std::memset(ocode.get(), 0x55, T);
      abn::sites_merge_serial(xchunks.get(), (int)chunks.size(), ins, filter,
                              abn::MergeOut{ochrom.get(), ostart.get(), oend.get(), ostrand.get(), ocode.get(), olevel.get()},
                              dr.get(), di.get());
      long long r = 0, j = 0;
      for (long long i = 0; i < n_lines; ++i) {
        const Line& l = file[(size_t)i];
        if (l.kind != Record && l.kind != Accepted) continue;
        const long long d = l.kind == Record ? dr[(size_t)r++] : di[(size_t)j++], k = place[(size_t)i];
        const uint8_t code = (uint8_t)(l.status | (l.pm < filter ? 0x80u : 0u));
        if (d != k || ochrom[(size_t)k] != l.chromosome || ostart[(size_t)k] != l.start || oend[(size_t)k] != l.end ||
            ostrand[(size_t)k] != l.strand || ocode[(size_t)k] != code || std::memcmp(&olevel[(size_t)k], &l.ml, 8) != 0) {
          std::printf("iteration %d, chunks of %lld lines: line %lld went to %lld, not %lld, or its fields differ\n", it,
                      chunk_lines, i, d, k);
          return 1;
        }
        nan_codes += l.pm != l.pm;
      }
    }
  }
  if (!records || !inserted || !rejected || !empty_chunks || !nan_codes) {
    std::printf("the cases miss a pattern: %zu %zu %zu %zu %zu\n", records, inserted, rejected, empty_chunks, nan_codes);
    return 1;
  }
  std::printf("sanitized sites merge ok: %zu records, %zu inserted, %zu rejected, %zu chunks without a record\n", records,
              inserted, rejected, empty_chunks);
  return 0;
}
