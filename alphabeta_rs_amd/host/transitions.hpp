// transitions.hpp — what `--transitions` adds to the two command-line tools: the 3 x 3 state transition table of every
// pair of sampled nodes (abn_pairwise_transitions*, include/abneutral.h; the joint table behind src/pedigree.rs:236-257)
// beside the pedigree, and its two output formats.  Nothing here runs without the flag.
#pragma once
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "alphabeta.hpp"

namespace alphabeta {
namespace transitions {

// the sampled nodes of a pedigree build, in the nodes' order, and their tables in the reference's pair order
struct Table {
  std::vector<std::string> names;
  std::vector<uint32_t> generations;
  std::vector<uint64_t> counts;  // [tables x pairs x 9]; tables: 1 (alphabeta) or the tiles / pools (metaprofile_alphabeta)
  size_t pairs() const { return names.size() * (names.size() - 1) / 2; }
};

// What a pedigree build is asked to leave behind: with `wanted` every build of the process appends its table (the runs
// of several --contexts in the order of the contexts).
struct Request {
  bool wanted = false;
  std::vector<Table> tables;
};
inline Request& request() {
  static Request r;
  return r;
}

inline void open_or_throw(std::FILE* f, const std::string& path) {
  if (!f) throw Error(ABN_ERR_INVALID_ARG, "could not write " + path);
}

// sample_a sample_b generation_a generation_b of every pair, one line each, behind `header` (may be empty)
inline void write_pairs(std::FILE* f, const Table& t, const uint64_t* counts) {
  size_t p = 0;
  for (size_t a = 0; a < t.names.size(); ++a)
    for (size_t b = a + 1; b < t.names.size(); ++b, ++p) {
      std::fprintf(f, "%s\t%s\t%u\t%u", t.names[a].c_str(), t.names[b].c_str(), t.generations[a], t.generations[b]);
      for (int e = 0; counts && e < 9; ++e) std::fprintf(f, "\t%llu", (unsigned long long)counts[9 * p + e]);
      std::fputc('\n', f);
    }
}

// <output>/transitions.txt of `alphabeta --transitions`
inline void write_txt(const std::string& path, const Table& t) {
  std::FILE* f = std::fopen(path.c_str(), "w");
  open_or_throw(f, path);
  std::fputs("sample_a\tsample_b\tgeneration_a\tgeneration_b\tUU\tUI\tUM\tIU\tII\tIM\tMU\tMI\tMM\n", f);
  write_pairs(f, t, t.counts.data());
  std::fclose(f);
}

// transition_pairs.txt and transitions.npy (NPY v1, <u8, C order, (tables, pairs, 9)) of `metaprofile_alphabeta --transitions`
inline void write_npy(const std::string& dir, const Table& t) {
  const std::string pairs_path = dir + "/transition_pairs.txt", npy_path = dir + "/transitions.npy";
  std::FILE* f = std::fopen(pairs_path.c_str(), "w");
  open_or_throw(f, pairs_path);
  write_pairs(f, t, nullptr);
  std::fclose(f);
  const size_t pairs = t.pairs(), tables = pairs ? t.counts.size() / (9 * pairs) : 0;
  std::string head = "{'descr': '<u8', 'fortran_order': False, 'shape': (" + std::to_string(tables) + ", " +
                     std::to_string(pairs) + ", 9), }";
  while ((10 + head.size() + 1) % 64 != 0) head += ' ';
  head += '\n';
  f = std::fopen(npy_path.c_str(), "wb");
  open_or_throw(f, npy_path);
  const unsigned char magic[10] = {0x93, 'N', 'U', 'M', 'P', 'Y', 1, 0, (unsigned char)(head.size() & 0xff),
                                   (unsigned char)(head.size() >> 8)};
  std::fwrite(magic, 1, 10, f);
  std::fwrite(head.data(), 1, head.size(), f);
  if (!t.counts.empty()) std::fwrite(t.counts.data(), sizeof(uint64_t), t.counts.size(), f);  // (little-endian hosts)
  std::fclose(f);
}

}  // namespace transitions
}  // namespace alphabeta
