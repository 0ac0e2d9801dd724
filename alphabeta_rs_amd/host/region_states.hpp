// region_states.hpp — `--region-states LO,HI [--region-min-sites K]`: region-level epimutation analysis.  Every tile of
// --tiles or row of --regions gets ONE state per sample, called on the device from the sample's sites inside it
// (abn_tiles_region_states; the law: csrc/abn_regions.hpp), and the pedigree is built from the regions' states: all regions
// in one group, or with --pool one group — one pedigree — per name in the list's 4th field.  Here: the flag's arguments as
// exact rationals, and the side files' array writer.  The run itself: tiles.hpp, regions_of_tiles.
#pragma once

#include <cstdint>
#include <fstream>
#include <string>
#include <vector>

namespace alphabeta {
namespace metaprofile {

constexpr int64_t kRegionDen = 1000000;  // LO and HI are read over 10^6: at most six fraction digits, no strtod
constexpr const char* kRegionStatesExpects =
    "--region-states expects LO,HI: two decimals in [0, 1] with at most six fraction digits, LO <= HI";

struct RegionArgs {
  bool wanted = false;
  int64_t lo_num = 0, hi_num = 0;  // over kRegionDen
  int64_t min_sites = 1;           // --region-min-sites K
};

// a decimal in [0, 1] with at most six fraction digits -> its numerator over 10^6; digits[.digits], either side may be
// empty but not both; no sign, no exponent, no blanks
inline bool parse_region_level(const std::string& t, int64_t& num) {
  const size_t dot = t.find('.');
  const std::string whole = t.substr(0, dot), frac = dot == std::string::npos ? std::string() : t.substr(dot + 1);
  if ((whole.empty() && frac.empty()) || whole.size() > 9 || frac.size() > 6) return false;
  int64_t w = 0, f = 0;
  for (char ch : whole) {
    if (ch < '0' || ch > '9') return false;
    w = w * 10 + (ch - '0');
  }
  for (char ch : frac) {
    if (ch < '0' || ch > '9') return false;
    f = f * 10 + (ch - '0');
  }
  for (size_t k = frac.size(); k < 6; ++k) f *= 10;
  num = w * kRegionDen + f;
  return num <= kRegionDen;
}
// the value of --region-states, or false
inline bool parse_region_states(const std::string& v, RegionArgs& out) {
  const size_t comma = v.find(',');
  if (comma == std::string::npos || v.find(',', comma + 1) != std::string::npos) return false;
  if (!parse_region_level(v.substr(0, comma), out.lo_num) || !parse_region_level(v.substr(comma + 1), out.hi_num)) return false;
  return out.lo_num <= out.hi_num;
}

// the value of --region-min-sites: decimal digits alone (no sign, no blank), from 1 to 10^18, or false
inline bool parse_region_min_sites(const std::string& v, int64_t& out) {
  if (v.empty() || v.size() > 18) return false;
  int64_t n = 0;
  for (char ch : v) {
    if (ch < '0' || ch > '9') return false;
    n = n * 10 + (ch - '0');
  }
  if (n < 1) return false;
  out = n;
  return true;
}

// ndarray_npy::write_npy of a uint8 (rows, cols) array, C order
inline void write_u8_npy(const std::vector<uint8_t>& a, size_t rows, size_t cols, const std::string& path) {
  std::string dict = "{'descr': '|u1', 'fortran_order': False, 'shape': (" + std::to_string(rows) + ", " + std::to_string(cols) + "), }";
  const size_t total = 10 + dict.size() + 1;
  dict += std::string((64 - total % 64) % 64, ' ') + "\n";
  std::ofstream f(path, std::ios::binary);
  const char magic[8] = {'\x93', 'N', 'U', 'M', 'P', 'Y', 1, 0};
  f.write(magic, 8);
  const uint16_t hl = (uint16_t)dict.size();
  f.write(reinterpret_cast<const char*>(&hl), 2);
  f.write(dict.data(), (std::streamsize)dict.size());
  f.write(reinterpret_cast<const char*>(a.data()), (std::streamsize)a.size());
}

}  // namespace metaprofile
}  // namespace alphabeta
