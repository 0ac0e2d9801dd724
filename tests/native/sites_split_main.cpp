// The partition of a resident methylome by context (alphabeta_rs_amd/csrc/abn_sites_split.hpp) in its serial form, built
// with -fsanitize=address,undefined by tests/test_sites_split_cpu.py: every array a heap block of exactly its length (a
// child's chunk holds exactly the records the scan promised it), against a filter by membership, record for record.
#include <cstdio>
#include <cstring>
#include <memory>
#include <random>
#include <vector>

#include "../../alphabeta_rs_amd/csrc/abn_sites_split.hpp"

using namespace abn;

namespace {

struct Block {  // six arrays of exactly n entries
  std::unique_ptr<uint32_t[]> line, meta, start, end;
  std::unique_ptr<double[]> pm, ml;
  long long n = 0;
  explicit Block(long long count = 0) : n(count) {
    const size_t k = (size_t)count;
    line.reset(new uint32_t[k]), meta.reset(new uint32_t[k]), start.reset(new uint32_t[k]), end.reset(new uint32_t[k]);
    pm.reset(new double[k]), ml.reset(new double[k]);
  }
};

int fail(const char* what, long long a, long long b, long long c) {
  std::printf("FAILED: %s (%lld, %lld, %lld)\n", what, a, b, c);
  return 1;
}

// chunk_n records per chunk, each with the code codes(rng) gives, under the parent's mask `contexts` (a record of a context
// outside it does not occur: the parse accepted none); 0 when the partition is the filter
template <class Codes>
int run_masked(const std::vector<long long>& chunk_n, uint32_t contexts, Codes codes, std::mt19937_64& rng,
               long long* moved) {
  const int n_chunks = (int)chunk_n.size();
  std::vector<Block> src;
  std::vector<SplitChunk> chunks((size_t)n_chunks);
  long long n_blocks = 0, before = 0, line0 = 0;
  for (int c = 0; c < n_chunks; ++c) {
    src.emplace_back(chunk_n[(size_t)c]);
    Block& b = src.back();
    for (long long i = 0; i < b.n; ++i) {
      uint32_t code = codes(rng);
      while (code != 3u && !((contexts >> code) & 1u)) code = (code + 1u) % 3u;
      b.line[(size_t)i] = (uint32_t)(2 * i + 1);
      b.meta[(size_t)i] = (uint32_t)(rng() % 258) | (uint32_t)(rng() % 3) << 16 | (uint32_t)(rng() % 3) << 20 |
                          (uint32_t)(rng() % 16 == 0) << 24 | code << kMetaContextShift;
      b.start[(size_t)i] = (uint32_t)rng();
      b.end[(size_t)i] = (uint32_t)rng();
      b.pm[(size_t)i] = (double)(rng() % 10000) / 1e4;
      b.ml[(size_t)i] = (double)(rng() % 10000) / 1e4;
    }
    const long long n_lines = 2 * b.n + 3;
    chunks[(size_t)c].src = MergeChunk{b.line.get(), b.meta.get(), b.start.get(), b.end.get(), b.pm.get(), b.ml.get(),
                                       b.n,          line0,        n_lines,       before};
    chunks[(size_t)c].block0 = n_blocks;
    n_blocks += split_blocks(b.n);
    before += b.n;
    line0 += n_lines;
  }
  for (long long b = 0; b < n_blocks; ++b) {  // every workgroup finds its chunk, and lies inside it
    const int c = split_chunk_of_block(chunks.data(), n_chunks, b);
    if (c < 0 || c >= n_chunks || b < chunks[(size_t)c].block0 ||
        b >= chunks[(size_t)c].block0 + split_blocks(chunks[(size_t)c].src.n))
      return fail("split_chunk_of_block", b, c, n_blocks);
  }
  const long long stride = n_blocks + 1;
  std::unique_ptr<uint32_t[]> count(new uint32_t[(size_t)(kSplitChildren * stride)]);
  std::memset(count.get(), 0xff, sizeof(uint32_t) * (size_t)(kSplitChildren * stride));
  split_count_serial(chunks.data(), n_chunks, contexts, count.get(), stride);
  split_scan_serial(count.get(), n_blocks, stride);
  std::vector<Block> out;  // child k's chunk c at c * 3 + k
  out.reserve((size_t)n_chunks * kSplitChildren);
  for (int c = 0; c < n_chunks; ++c)
    for (int k = 0; k < kSplitChildren; ++k) {
      out.emplace_back((long long)split_chunk_size(chunks.data(), n_chunks, c, k, count.get(), stride, n_blocks));
      Block& b = out.back();
      chunks[(size_t)c].out[k] = SplitOut{b.line.get(), b.meta.get(), b.start.get(), b.end.get(), b.pm.get(), b.ml.get()};
    }
  split_scatter_serial(chunks.data(), n_chunks, contexts, count.get(), stride, n_blocks);
  for (int c = 0; c < n_chunks; ++c)
    for (int k = 0; k < kSplitChildren; ++k) {
      const Block &s = src[(size_t)c], &o = out[(size_t)c * kSplitChildren + k];
      long long at = 0;
      for (long long i = 0; i < s.n; ++i) {
        const uint32_t code = meta_context(s.meta[(size_t)i]);
        if (!(code == 3u || code == (uint32_t)k) || !((contexts >> k) & 1u)) continue;
        if (at >= o.n) return fail("a child's chunk is too short", c, k, at);
        if (o.line[(size_t)at] != s.line[(size_t)i] || o.meta[(size_t)at] != s.meta[(size_t)i] ||
            o.start[(size_t)at] != s.start[(size_t)i] || o.end[(size_t)at] != s.end[(size_t)i] ||
            std::memcmp(&o.pm[(size_t)at], &s.pm[(size_t)i], 8) || std::memcmp(&o.ml[(size_t)at], &s.ml[(size_t)i], 8))
          return fail("a record out of place", c, k, at);
        ++at;
      }
      if (at != o.n) return fail("a child's chunk is too long", c, k, at);
      *moved += at;
    }
  // a flagged line's children: the record's membership; a line without a record has none
  for (int c = 0; c < n_chunks; ++c) {
    const MergeChunk& m = chunks[(size_t)c].src;
    for (long long i = 0; i < m.n; i += 37) {
      if (split_flagged_membership(m, m.line0 + m.line[i], contexts) != split_membership(m.meta[i], contexts))
        return fail("split_flagged_membership", c, i, 0);
      if (split_flagged_membership(m, m.line0 + m.line[i] + 1, contexts) != 0u)
        return fail("a line without a record", c, i, 0);
    }
  }
  return 0;
}

// the case under every mask of two or three contexts
template <class Codes>
int run_case(const std::vector<long long>& chunk_n, Codes codes, std::mt19937_64& rng, long long* moved) {
  for (uint32_t contexts : {3u, 5u, 6u, 7u})
    if (run_masked(chunk_n, contexts, codes, rng, moved)) return 1;
  return 0;
}

}  // namespace

int main() {
  std::mt19937_64 rng(20240607);
  long long moved = 0, cases = 0;
  const long long counts[] = {0, 1, 255, 256, 257, 1025};
  auto any = [](std::mt19937_64& r) { return (uint32_t)(r() % 4); };
  auto mostly_chh = [](std::mt19937_64& r) { return (uint32_t)(r() % 10 < 7 ? 2 : r() % 4); };
  auto no_chg = [](std::mt19937_64& r) { return (uint32_t)(r() % 2 ? 0 : 2); };
  auto rows_only = [](std::mt19937_64&) { return 3u; };
  auto cg_only = [](std::mt19937_64&) { return 0u; };
  for (long long n : counts) {  // one chunk of every count
    if (run_case({n}, any, rng, &moved) || run_case({n}, mostly_chh, rng, &moved) || run_case({n}, no_chg, rng, &moved) ||
        run_case({n}, rows_only, rng, &moved) || run_case({n}, cg_only, rng, &moved))
      return 1;
    cases += 5;
  }
  for (long long a : counts)  // several chunks, empty ones in front, between and behind
    for (long long b : counts) {
      if (run_case({a, b}, any, rng, &moved) || run_case({a, 0, b, 0}, mostly_chh, rng, &moved) ||
          run_case({0, 0, a, b, 3, 0, 700}, no_chg, rng, &moved) || run_case({a, b, a}, rows_only, rng, &moved))
        return 1;
      cases += 4;
    }
  for (int seed = 0; seed < 60; ++seed) {  // many small chunks, as a small slab size cuts them
    std::vector<long long> chunk_n;
    const int n_chunks = 1 + (int)(rng() % 40);
    for (int c = 0; c < n_chunks; ++c) chunk_n.push_back((long long)(rng() % 4 == 0 ? 0 : rng() % 600));
    if (run_case(chunk_n, any, rng, &moved)) return 1;
    ++cases;
  }
  if (run_case({}, any, rng, &moved)) return 1;  // a handle without a chunk
  std::printf("sanitized sites split ok: %lld cases, %lld records placed\n", cases + 1, moved);
  return 0;
}
