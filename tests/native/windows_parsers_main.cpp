// Stand-alone driver for the host parsers of the window extraction (alphabeta_rs_amd/host/windows_extract.hpp), built by
// tests/test_windows_host.py with AddressSanitizer + UndefinedBehaviorSanitizer and run directly: the annotation given as
// argv[1] and a methylome synthesised against it, intact, then truncated and corrupted (seeded), through
// parse_annotation, parse_site_full, choose_genes and window_params.  Whatever the text, the parsers answer with lists
// and arrays of consistent sizes, never with a sanitizer report.  No device: nothing here touches abn_*.
#include <cstdio>

#include "../../alphabeta_rs_amd/host/alphabeta.hpp"

namespace w = alphabeta::windows;

static uint64_t rng_state = 20261018ull;
static uint32_t rnd(uint32_t n) {
  rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
  return n ? (uint32_t)(rng_state >> 33) % n : 0;
}

static std::string corrupt(std::string s) {
  static const char* junk[] = {"", "\t", " ", "*", "+", "-", "chr", "chrchrM", "C", "256", "4294967295", "4294967296",
                               "-1", "1e999", "nan", "CG", "\r\n", "\n\n", "\xff\xfe", "0x10", "+5", "99999999999999999999"};
  const size_t njunk = sizeof junk / sizeof *junk;
  switch (rnd(7)) {
    case 0: return s.substr(0, rnd((uint32_t)s.size() + 1));  // cut anywhere, mid-field included
    case 1: return "";
    case 2:
      for (int k = 0; k < 8 && !s.empty(); ++k) s[rnd((uint32_t)s.size())] = (char)rnd(256);
      return s;
    case 3: {
      for (int k = 0; k < 6 && !s.empty(); ++k) s.insert(rnd((uint32_t)s.size()), junk[rnd((uint32_t)njunk)]);
      return s;
    }
    case 4: {  // fields dropped: tabs become spaces or vanish
      for (auto& c : s)
        if (c == '\t' && rnd(20) == 0) c = rnd(2) ? ' ' : 'x';
      return s;
    }
    case 5: {
      for (auto& c : s)
        if (c == '\n' && rnd(10) == 0) c = '\t';
      return s;
    }
    default: return s + s.substr(0, rnd((uint32_t)s.size() + 1));
  }
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const std::string annotation = alphabeta::detail::read_file(argv[1], "annotation");
  const w::Genome g0 = w::parse_annotation(annotation);
  if (g0.n_genes != 100) return std::printf("annotation: %zu genes\n", g0.n_genes), 1;
  // a methylome with sites around every gene of the annotation, all formats
  std::string methylome = "seqnames\tstart\tstrand\tcontext\tcounts.methylated\tcounts.total\tposteriorMax\tstatus\trc.meth.lvl\n";
  for (const auto& kv : g0.chromosomes)
    for (const auto& gene : kv.second.combined)
      for (uint32_t p = gene.start > 30 ? gene.start - 30 : 0; p < gene.start + 60; p += 7) {
        const std::string c = std::to_string(kv.first), ps = std::to_string(p);
        switch (p % 4) {
          case 0: methylome += c + "\t" + ps + "\t+\tCG\t1\t8\t0.9999\tM\t0.75\n"; break;
          case 1: methylome += "chr" + c + "\t" + ps + "\t-\tCG\t1\t8\t0.5\tU\t0.01\tCGA\n"; break;
          case 2: methylome += c + "\t" + ps + "\t" + std::to_string(p + 2) + "\tCG\tx\t+\t1\t8\t0.9999\tI\t0.5\n"; break;
          default: methylome += c + " " + ps + " " + std::to_string(p + 3) + " E10\n"; break;
        }
      }
  const w::GeneRule rules[2] = {{2048, false}, {0, true}};
  size_t sites = 0, with_gene = 0, cases = 0;
  std::string warnings;  // "invalid methylation status" lines: kept off stdout
  alphabeta::detail::diag_sink() = &warnings;
  for (int it = 0; it < 200; ++it) {
    warnings.clear();
    const std::string a = it == 0 ? annotation : (rnd(3) ? corrupt(annotation) : annotation);
    const std::string m = it == 0 ? methylome : corrupt(methylome);
    const w::Genome g = w::parse_annotation(a);
    for (const auto& rule : rules) {
      const w::SampleSites s = w::choose_genes(m, g, rule, 0.99);
      if (s.gene_start.size() != s.size() || s.gene_end.size() != s.size() || s.flags.size() != s.size() ||
          s.code.size() != s.size() || s.level.size() != s.size())
        return std::printf("ragged arrays\n"), 1;
      sites += s.size();
      for (uint8_t f : s.flags) with_gene += (f >> 1) & 1;
      ++cases;
    }
    const abn_windows_params p = w::window_params(rnd(5000), 1 + rnd(300), rnd(300), rnd(2) != 0, g.max_gene_length);
    if (p.n_upstream < 0 || p.n_gene < 0) return std::printf("negative window count\n"), 1;
  }
  if (with_gene == 0 || with_gene == sites) return std::printf("one outcome only\n"), 1;
  std::printf("sanitized windows ok %zu %zu %zu\n", cases, sites, with_gene);
  return 0;
}
