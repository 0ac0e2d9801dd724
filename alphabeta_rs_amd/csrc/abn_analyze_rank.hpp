// The key and rank arithmetic of the device analysis (abn_analyze.hpp; src/analysis.rs:50-98): the order-preserving
// 64-bit key of a double that the radix select sorts by, and which order statistics the Linear quantile of
// ndarray-stats reads.  Plain arithmetic, no HIP header: the kernel, abn_analyze's mirror on the host and the CPU tests
// (tests/test_analyze_rank_cpu.py) all include this file as it is.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ABN_HOST_DEVICE __host__ __device__
#else
#define ABN_HOST_DEVICE
#endif

namespace abn {

// double -> key: a < b (as doubles, neither NaN) implies key(a) < key(b) as unsigned integers.  A non-negative double's
// bits already grow with its value (subnormals and +inf included): set the sign bit to lift them above the negatives.
// A negative double's bits grow as the value falls: invert all of them.  -0.0 and +0.0, which `<` ties, get the
// adjacent keys 0x7fff...f and 0x8000...0: -0.0 sorts first.  That is one of the placements abn_analyze's std::sort
// may choose, and the quantile does not depend on the choice: s[lo] + frac * (s[hi] - s[lo]) with frac in [0, 1) gives
// +0.0 whenever both operands are zeros of either sign (x - y of equal-magnitude zeros is +0.0 or, for -0 - +0, -0.0;
// frac times that is a zero; a zero plus a zero of the other sign is +0.0; and -0 + frac * (-0 - -0) = -0 + +0 = +0.0),
// and where one operand is not a zero the sign of the other, a zero, changes neither the difference nor the sum
// (tests/test_analyze_rank_cpu.py tries every placement).  NaN has no place in the order: the analysis refuses a table
// with one before any key is compared.
ABN_HOST_DEVICE inline uint64_t abn_f64_bits(double x) {
  uint64_t u;
  memcpy(&u, &x, sizeof u);
  return u;
}
ABN_HOST_DEVICE inline uint64_t abn_order_key(double x) {
  const uint64_t u = abn_f64_bits(x), sign = 0x8000000000000000ull;
  return (u & sign) ? ~u : (u | sign);
}
ABN_HOST_DEVICE inline double abn_order_key_value(uint64_t key) {
  const uint64_t sign = 0x8000000000000000ull, u = (key & sign) ? (key ^ sign) : ~key;
  double x;
  memcpy(&x, &u, sizeof x);
  return x;
}

// QuantileExt::quantile_axis_mut with Linear (src/analysis.rs:60-97; abn_analyze, csrc/abn_analyze.hip): quantile q of
// n_boot values reads the ascending order statistics lo = floor(fi) and hi = ceil(fi), fi = q (n_boot - 1), and
// interpolates with frac = fi - trunc(fi): s[lo] + frac * (s[hi] - s[lo]).  hi is lo or lo + 1.
struct QuantileRank {
  int64_t lo, hi;
  double frac;
};
ABN_HOST_DEVICE inline QuantileRank abn_quantile_rank(double q, int64_t n_boot) {
  const double fi = q * (double)(n_boot - 1);
  QuantileRank r;
  r.lo = (int64_t)__builtin_floor(fi);
  r.hi = (int64_t)__builtin_ceil(fi);
  r.frac = fi - __builtin_trunc(fi);
  return r;
}
ABN_HOST_DEVICE inline double abn_quantile_interpolate(double s_lo, double s_hi, double frac) {
  return s_lo + frac * (s_hi - s_lo);
}

// the NaN test of RawAnalysis::analyze (host/alphabeta.hpp) on one bootstrap row of seven: a NaN entry or a NaN
// beta / alpha (src/analysis.rs:54).  isnan only: +-inf is not refused.
ABN_HOST_DEVICE inline bool abn_analyze_row_is_bad(const double* row) {
  const double ratio = row[1] / row[0];
  bool bad = ratio != ratio;
  for (int k = 0; k < 7; ++k) bad = bad || row[k] != row[k];
  return bad;
}

// the two quantiles of the confidence interval (src/analysis.rs:60-97)
ABN_HOST_DEVICE inline double abn_analyze_quantile(int which) { return which == 0 ? 0.025 : 0.975; }
// table column of each output column (alpha, beta, beta/alpha, weight, intercept, PrMM, PrUM, PrUU); -1: beta / alpha
ABN_HOST_DEVICE inline int abn_analyze_source_column(int k) { return k < 2 ? k : (k == 2 ? -1 : k - 1); }

}  // namespace abn
