// Stand-alone driver for the line parser host and device share (alphabeta_rs_amd/csrc/abn_parse.hpp), built by
// tests/test_parse_cpu.py with AddressSanitizer + UndefinedBehaviorSanitizer and run directly.  Seeded methylome lines of
// every format, intact and corrupted, each copied into a heap block of exactly its length (a read past either end of the
// byte range is a report), through abn_parse_line — and through the host's parse_site_full, which must agree wherever the
// shared parser does not defer.  No device: nothing here touches abn_*.
#include <cstdio>
#include <memory>

#include "../../alphabeta_rs_amd/csrc/abn_parse.hpp"
#include "../../alphabeta_rs_amd/host/alphabeta.hpp"

namespace w = alphabeta::windows;

static uint64_t rng_state = 20261018ull;
static uint32_t rnd(uint32_t n) {
  rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
  return n ? (uint32_t)(rng_state >> 33) % n : 0;
}

int main() {
  static const char* junk[] = {"", "\t", " ", "*", "+", "-", "chr", "chrchrM", "C", "256", "4294967295", "4294967296", "-1",
                               "1e999", "nan", "inf", "CG", "\r", "\xff\xfe", "0x10", "+5", "99999999999999999999", ".",
                               "e", "E-", "1e22", "1e-23", "9007199254740993", "0.00000000000000000000001", "-0.0"};
  const size_t njunk = sizeof junk / sizeof *junk;
  std::string warnings;
  alphabeta::detail::diag_sink() = &warnings;
  size_t sites = 0, none = 0, deferred = 0;
  for (int it = 0; it < 200000; ++it) {
    const std::string c = std::to_string(rnd(300)), p = std::to_string(rnd(4000000)), v = "0." + std::to_string(rnd(10000));
    std::string s;
    switch (rnd(4)) {
      case 0: s = c + "\t" + p + "\t+\tCG\t1\t8\t" + v + "\tM\t0.75"; break;
      case 1: s = "chr" + c + "\t" + p + "\t-\tCG\t1\t8\t0.5\tU\t" + v + "\tCGA"; break;
      case 2: s = c + "\t" + p + "\t" + p + "\tCG\tx\t+\t1\t8\t" + v + "\tI\t1e-3"; break;
      default: s = c + " " + p + "\t" + p + " E10"; break;
    }
    for (int k = (int)rnd(4); k > 0 && !s.empty(); --k) {
      switch (rnd(4)) {
        case 0: s.insert(rnd((uint32_t)s.size() + 1), junk[rnd((uint32_t)njunk)]); break;
        case 1: s[rnd((uint32_t)s.size())] = (char)rnd(256); break;
        case 2: s.erase(rnd((uint32_t)s.size()), 1 + rnd(3)); break;
        default: s = s.substr(0, rnd((uint32_t)s.size() + 1)); break;
      }
    }
    std::unique_ptr<unsigned char[]> block(new unsigned char[s.size()]);  // exactly the line: no terminator behind it
    std::memcpy(block.get(), s.data(), s.size());
    const unsigned char* b = block.get();
    const unsigned char* e = abn::abn_line_trim(b, b + s.size());
    abn::ParsedSite got{};
    const int cls = abn::abn_parse_line(b, e, got);
    w::FullSite want{};
    warnings.clear();
    const bool is_site = w::parse_site_full(std::string((const char*)b, (size_t)(e - b)), want);
    if (cls == abn::kLineDeferred) {
      ++deferred;
      continue;
    }
    if ((cls == abn::kLineSite) != is_site) return std::printf("class differs: %s\n", s.c_str()), 1;
    if (!is_site) {
      ++none;
      continue;
    }
    ++sites;
    if (got.chromosome != want.chromosome || got.start != want.start || got.end != want.end ||
        got.strand != (uint32_t)want.strand || got.status != want.status_numeric ||
        std::memcmp(&got.posteriormax, &want.posteriormax, 8) || std::memcmp(&got.meth_lvl, &want.meth_lvl, 8) ||
        (got.status_flag != 0) != !warnings.empty())
      return std::printf("record differs: %s\n", s.c_str()), 1;
  }
  if (!sites || !none || !deferred) return std::printf("one outcome only\n"), 1;
  std::printf("sanitized parse ok %zu %zu %zu\n", sites, none, deferred);
  return 0;
}
