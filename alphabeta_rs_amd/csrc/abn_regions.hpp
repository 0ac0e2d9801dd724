// Region-level methylation states: one 2-bit field per (sample, region) called from the sample's single-site fields inside
// the region, written in the packed format of abn_pack_codes, so that every packed scan and the census take the result as
// they take a matrix of sites.  Plain arithmetic, no HIP header: the law, the lane function, the serial form and the walk
// of the kernel's lane structure compile with a host compiler (tests/native/regions_main.cpp); the kernel only where
// abn_regions.hip asks for it (ABN_REGIONS_KERNELS).
//
// THE LAW.  Inputs: a packed matrix of n rows and L sites (site 4 j + e of a dword is byte e, bits 2j..2j+1; field 3 =
// filtered); T windows [begin[t], end[t]), any column ranges of the rows, overlapping or empty; a column map src[C] with
// src[c] in [0, T), repeats and omissions allowed (NULL: the identity, C = T); a rule of exact integers lo_num, hi_num,
// den, min_kept with 0 <= lo_num <= hi_num <= den, 1 <= den <= 2^20, min_kept >= 1.  For sample s and window t let n0, n1,
// n2 be the fields 0, 1, 2 of row s inside the window (what abn_packed_census_windows counts), kept = n0 + n1 + n2 and
// m = n1 + 2 n2 — twice the sum of state / 2, the level abn_sim_pedigree and abn_sim_study use.  The region's field is
//     3  if kept < min_kept (an empty window is always 3),
//     0  if m den < lo_num 2 kept,
//     2  if m den > hi_num 2 kept,
//     1  otherwise (equality on either side is 1).
// All in 64-bit unsigned arithmetic: a row holds L <= 2^34 sites, so m <= 2^35 and 2 kept <= 2^35; with den, lo_num,
// hi_num <= 2^20 both products stay below 2^56.  No floating point anywhere.  Output: n rows of abn_packed_row_stride(C)
// bytes; column c of row s holds the field of window src[c]; the fields from C to the end of the stride are 3.
//
// MAPPING (abn_region_states_kernel).  One lane per (row, output column); 16 consecutive lanes own one output dword; a
// workgroup of 256 lanes owns one 64-byte super-step of one output row; the grid is (row_stride_out / 64, n), so every
// byte of the output is written exactly once, padding fields (columns >= C call 3) by the same lanes, and a wavefront's
// four dwords go out as one 16-byte run of a row.  C <= INT32_MAX and n <= 65535 keep both grid dimensions legal without
// a grid stride.  A lane reads t = src[c] and the window's record, walks the dwords begin >> 4 .. (end - 1) >> 4 of its
// row with the first and the last masked (abn_packed_window_mask: a field outside reads as 3), counts with census_dword in
// 32-bit registers — only windows below long_sites < 2^30 sites are walked — and calls the rule.
//   The sixteen fields of a dword are combined by four xor shuffles (8, 4, 2, 1) inside each group of 16 lanes: every lane
// shifts its field to its place in the dword — (f << (8 e + 2 j)) for column 4 j + e — and the group ORs.  Ballots would
// give two 64-bit masks per wavefront in LANE order, which the format's byte-interleaved order (site 4 j + e at bit 8 e +
// 2 j) would still have to be permuted into, per group; the shuffles put every field where it belongs with no permutation
// and cost four cross-lane steps (ds_bpermute_b32: the LDS crossbar, no LDS allocated) next to a walk of global loads.  No
// LDS, no atomics, no scratch.
//   Neighbouring lanes normally hold neighbouring tiles, so their 4-byte loads fall into the same or adjacent cache lines
// of one row and a wavefront's trip touches a few lines.  Under a permuting src that locality is the permutation's: the
// result is the same, each lane's loads are still sequential in its own window, but a wavefront's trip may touch up to 64
// lines.  The record loads (src, the window) stay coalesced in either case.
//
// LONG WINDOWS.  A lane with a 40 000-site window would hold its wavefront for thousands of trips.  Windows of at least
// long_sites sites are counted beforehand by the census kernels (abn_packed_census.hpp; one launch over just those
// windows) into a table uint64 [K x n x 3]; the window's record then carries the table's row in place of a range
// (RegionWindow: begin = -1 - k), and the lane takes its three counts from there and reads no field.
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

#include "abn_packed_census.hpp"

namespace abn {

constexpr int kRegionThreads = 256;     // one 64-byte super-step of one output row
constexpr int kRegionDwordLanes = 16;   // the lanes of one output dword
// Windows of at least this many sites go through the census kernels.  A lane walks its window alone, 16 sites per 4-byte
// load, so a window of w sites keeps its wavefront for w / 16 trips; the census route spends a workgroup of 256 lanes and a
// second kernel's wavefront on every (window, sample) whatever the length.  Measured (docs/experiments.md, "Region states",
// 8 rows of 2 000 000 sites in equal tiles): the walked kernel is 172 to 2.1 times faster than abn_packed_census_windows_dev
// over the same windows at 8 to 1024 sites and level with it at 2048 (0.96); the two lines cross at about 2000 sites, which
// is this value to a multiple of 256.  (Census and table read together overtake the walk only between 2048 and 4096 sites
// when every window has one length; among short windows a long one also holds its whole wavefront, which that table does
// not show.)
constexpr long long kRegionLongSites = 2048;
constexpr long long kRegionLongSitesMax = 1ll << 29;  // a walked window's 32-bit counts
static_assert(kRegionLongSites % 16 == 0 && kRegionLongSites <= kRegionLongSitesMax, "whole dwords; 32-bit counts");

struct RegionRule {
  uint64_t lo_num, hi_num, den, min_kept;
};
// A window as a lane reads it: [begin, end), or (begin < 0) row -1 - begin of the long windows' table
struct RegionWindow {
  long long begin, end;
};

// the field of a region from its counts
ABN_HOST_DEVICE inline uint32_t region_call(uint64_t n0, uint64_t n1, uint64_t n2, const RegionRule r) {
  const uint64_t kept = n0 + n1 + n2;
  if (kept < r.min_kept) return 3u;
  const uint64_t a = (n1 + 2 * n2) * r.den, k2 = 2 * kept;  // both products below 2^56 (header)
  if (a < r.lo_num * k2) return 0u;
  if (a > r.hi_num * k2) return 2u;
  return 1u;
}

// What one lane counts of the window [begin, end), 0 <= begin <= end, end - begin < 2^30, of a row: load(d) is dword d of
// the row.  Reads the dwords begin >> 4 .. (end - 1) >> 4 and nothing else; none for an empty window.
template <class Load>
ABN_HOST_DEVICE inline void region_lane_count(Load load, long long begin, long long end, uint32_t& n0, uint32_t& n1,
                                              uint32_t& n2) {
  if (begin >= end) return;
  const long long d0 = begin >> 4, d1 = (end - 1) >> 4;
  for (long long d = d0; d <= d1; ++d) {
    uint32_t x = load(d);
    if (d == d0 || d == d1) x |= abn_packed_window_mask(0, (int)(begin - 16 * d), (int)(end - 16 * d));
    census_dword(x, n0, n1, n2);
  }
}
// where the field of output column c goes in its dword
ABN_HOST_DEVICE inline uint32_t region_field_at(uint32_t field, long long c) {
  const int k = (int)(c & 15);
  return field << (8 * (k & 3) + 2 * (k >> 2));
}

// the long-window default behind an argument of 0
inline long long region_long_sites(long long long_sites) { return long_sites == 0 ? kRegionLongSites : long_sites; }

// "" or why the arguments are refused: census_refusal's words, then the rule, the column map and long_sites
inline std::string region_refusal(const void* packed, int64_t n, int64_t n_sites, int64_t row_stride, const int64_t* begin,
                                  const int64_t* end, int64_t T, const int32_t* src, int64_t C, int64_t lo_num, int64_t hi_num,
                                  int64_t den, int64_t min_kept, int64_t long_sites, const void* out) {
  if (T > 0x7fffffffLL) return "more windows than INT32_MAX";
  if (C > 0x7fffffffLL) return "more columns than INT32_MAX";
  std::string why = census_refusal(packed, n, n_sites, row_stride, begin, end, T, packed);
  if (!why.empty()) return why;
  if (C < 0 || (C > 0 && !out)) return "null/size";
  if (den < 1 || den > (1ll << 20) || lo_num < 0 || lo_num > hi_num || hi_num > den)
    return "the rule is not 0 <= lo_num <= hi_num <= den with den in 1..2^20";
  if (min_kept < 1) return "min_kept is below 1";
  if (long_sites < 0 || long_sites % 16 != 0 || long_sites > kRegionLongSitesMax)
    return "long_sites is negative, not a multiple of 16, or above 2^29";
  if (!src && C != T) return "src is null and n_columns is not n_windows";
  if (src)
    for (int64_t c = 0; c < C; ++c)
      if (src[c] < 0 || src[c] >= T) return "column " + std::to_string(c) + ": src is not a window in 0.." + std::to_string(T - 1);
  return "";
}

// The serial form, field by field: out [n x out_stride], out_stride = abn_packed_row_stride(C) (at least), every field of
// the first abn_packed_row_stride(C) bytes of a row written
inline void region_states_serial(const uint8_t* packed, int64_t n, int64_t row_stride, const int64_t* begin, const int64_t* end,
                                 const int32_t* src, int64_t C, const RegionRule rule, uint8_t* out, int64_t out_stride) {
  const int64_t fields = (C + kPackedStepSites - 1) / kPackedStepSites * kPackedStepSites;
  for (int64_t s = 0; s < n; ++s) {
    const uint8_t* row = packed + s * row_stride;
    uint8_t* o = out + s * out_stride;
    for (int64_t b = 0; b < fields / 4; ++b) o[b] = 0;
    for (int64_t c = 0; c < fields; ++c) {
      uint32_t f = 3u;
      if (c < C) {
        const int64_t t = src ? src[c] : c;
        uint64_t cnt[4] = {0, 0, 0, 0};
        for (int64_t k = begin[t]; k < end[t]; ++k) ++cnt[(row[(k >> 4) * 4 + (k & 3)] >> (2 * ((k >> 2) & 3))) & 3];
        f = region_call(cnt[0], cnt[1], cnt[2], rule);
      }
      o[(c >> 4) * 4 + (c & 3)] |= (uint8_t)(f << (2 * ((c >> 2) & 3)));
    }
  }
}

// The windows as the kernel's lanes read them, and the long ones' ranges for the census: window t with at least
// long_sites (> 0) sites becomes row k of the table, in ascending t
inline void region_plan(const int64_t* begin, const int64_t* end, int64_t T, long long long_sites, std::vector<RegionWindow>& win,
                        std::vector<int64_t>& long_begin, std::vector<int64_t>& long_end) {
  win.resize((size_t)T);
  long_begin.clear(), long_end.clear();
  for (int64_t t = 0; t < T; ++t) {
    if (end[t] - begin[t] >= long_sites) {
      win[(size_t)t] = RegionWindow{-1 - (long long)long_begin.size(), 0};
      long_begin.push_back(begin[t]), long_end.push_back(end[t]);
    } else {
      win[(size_t)t] = RegionWindow{(long long)begin[t], (long long)end[t]};
    }
  }
}

// What the lane of (row s, output column c) calls: 3 for a padding column; the counts of its window from the table
// (`table` uint64 [K x n x 3]) or from its own walk
template <class Load>
ABN_HOST_DEVICE inline uint32_t region_lane_field(Load load, long long s, long long n, long long c, long long C,
                                                  const int32_t* src, const RegionWindow* win, const unsigned long long* table,
                                                  const RegionRule rule) {
  if (c >= C) return 3u;
  const RegionWindow w = win[src ? (long long)src[c] : c];
  if (w.begin < 0) {
    const unsigned long long* k = table + ((-1 - w.begin) * n + s) * 3;
    return region_call(k[0], k[1], k[2], rule);
  }
  uint32_t n0 = 0, n1 = 0, n2 = 0;
  region_lane_count(load, w.begin, w.end, n0, n1, n2);
  return region_call(n0, n1, n2, rule);
}

// The kernel's structure walked on the host: the plan, the long windows through the census's own walk, then every
// workgroup (super-step x row) of kRegionThreads lanes, each group of 16 ORing its fields into one dword.  long_sites > 0.
inline void region_states_walk(const uint8_t* packed, int64_t n, int64_t row_stride, const int64_t* begin, const int64_t* end,
                               int64_t T, const int32_t* src, int64_t C, const RegionRule rule, long long long_sites, uint8_t* out,
                               int64_t out_stride) {
  std::vector<RegionWindow> win;
  std::vector<int64_t> lb, le;
  region_plan(begin, end, T, long_sites, win, lb, le);
  const size_t K = lb.size();
  std::vector<uint64_t> table(K * (size_t)n * 3 + 1, 0);
  if (K > 0) {
    const std::vector<long long> chunk(K, kPmxWinPackedChunkSites);
    census_windows_walk(packed, n, row_stride, lb.data(), le.data(), (int64_t)K, chunk.data(), table.data());
  }
  const int64_t steps = (C + kPackedStepSites - 1) / kPackedStepSites;
  for (int64_t s = 0; s < n; ++s) {
    const uint8_t* row = packed + s * row_stride;
    const auto load = [row](long long d) {
      const uint8_t* at = row + 4 * d;
      return (uint32_t)at[0] | (uint32_t)at[1] << 8 | (uint32_t)at[2] << 16 | (uint32_t)at[3] << 24;
    };
    for (int64_t step = 0; step < steps; ++step)
      for (int group = 0; group < kRegionThreads / kRegionDwordLanes; ++group) {
        uint32_t dword = 0;
        for (int k = 0; k < kRegionDwordLanes; ++k) {
          const long long c = step * kRegionThreads + group * kRegionDwordLanes + k;
          dword |= region_field_at(region_lane_field(load, s, n, c, C, src, win.data(),
                                                     (const unsigned long long*)table.data(), rule), c);
        }
        uint8_t* o = out + s * out_stride + step * 64 + group * 4;
        for (int b = 0; b < 4; ++b) o[b] = (uint8_t)(dword >> (8 * b));
      }
  }
}

#if defined(__HIPCC__) && defined(ABN_REGIONS_KERNELS)  // (abn_regions.hip defines it)
// grid (out_stride / 64, n) of kRegionThreads lanes.  Bounds: c < C before src and win are read; src[c] in [0, T) and every
// window a column range of rows of n_sites <= 4 row_stride sites (the entries' checks), so dword (end - 1) >> 4 lies in the
// row; a long window's table row is below K; the output dword blockIdx.x * 16 + lane / 16 lies in a row of out_stride bytes.
__global__ void __launch_bounds__(kRegionThreads)
abn_region_states_kernel(const uint8_t* __restrict__ packed, long long row_stride, long long n, const int32_t* __restrict__ src,
                         const RegionWindow* __restrict__ win, const unsigned long long* __restrict__ table, long long C,
                         RegionRule rule, uint8_t* __restrict__ out, long long out_stride) {
  const long long s = blockIdx.y, c = (long long)blockIdx.x * kRegionThreads + threadIdx.x;
  const uint32_t* row = reinterpret_cast<const uint32_t*>(packed + (size_t)s * (size_t)row_stride);
  const uint32_t field = region_lane_field([row](long long d) { return row[d]; }, s, n, c, C, src, win, table, rule);
  uint32_t dword = region_field_at(field, c);
#pragma unroll
  for (int off = kRegionDwordLanes / 2; off > 0; off >>= 1) dword |= (uint32_t)__shfl_xor((int)dword, off, kRegionDwordLanes);
  if ((threadIdx.x & (kRegionDwordLanes - 1)) == 0)
    reinterpret_cast<uint32_t*>(out + (size_t)s * (size_t)out_stride)[c >> 4] = dword;
}
#endif

}  // namespace abn
